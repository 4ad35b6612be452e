// A TEXTUAL part of the quad march (quad_stage.h): #include it at the place of use, inside the loop over a thread's quads (why
// text and not a function: quad_part_warp.h; as a function it changed prolong_kernel).  No include guard.
//
// The store of a quad's four flow vectors from registers (prolong_kernel, median_march): two 16-byte buffer stores where the quad
// is whole; a row's ragged end leaves as one 8-byte store per pixel, because the bytes behind it are the next row's.  The stores
// go through rs_f, a buffer resource of exactly the field's w * h * 8 bytes.
//
// Reads   int x0, y, w, npx; float fu[4], fv[4]; the resource rs_f
// Defines uint32_t fo, the quad's byte offset in the field
const uint32_t fo = 8u * ((uint32_t)y * (uint32_t)w + (uint32_t)x0);
if (npx == 4) {
    f32x4 lo4, hi4;
    lo4[0] = fu[0], lo4[1] = fv[0], lo4[2] = fu[1], lo4[3] = fv[1];
    hi4[0] = fu[2], hi4[1] = fv[2], hi4[2] = fu[3], hi4[3] = fv[3];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t, lo4), rs_f, fo, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t, hi4), rs_f, fo, 16, 0);
} else {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < npx) {
            f32x2 p;
            p[0] = fu[k], p[1] = fv[k];
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t, p), rs_f, fo + 8u * k, 0, 0);
        }
}
