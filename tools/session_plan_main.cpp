// What a session is and where its buffers lie (csrc/session_plan.h) as a stand-alone host program: reads session descriptions from
// stdin, one per line, and prints each one's plan.  tests/test_session_plan.py builds and checks it.
//
//   session_plan_main [--summary] < descriptions
//
// A description is a line of NAME=VALUE words (a line without any is skipped).  The names are the fields of ofx_params (include/ofx.h;
// the six row arrays of a sharded session take one value per level, separated by commas) and the session's switches, iter_fused,
// iter_pairs, iter_dma, pair_pack, pair_waves and debug_corner_extent (ofx_plan::SessionSwitches).  What a line leaves out is 0,
// except window (9), mode (1: lk_float), levels (1) and the switches, which keep their defaults.
//
// Output per description, either "error CODE MESSAGE" or
//   plan NAME=VALUE ...                  the session's counts and flags, the effective borrow_frames / stream_two_stage, total
//   level K NAME=VALUE ...               geometry and byte sizes of level K
//   at NAME I J K OFFSET                 one line per pointer the session holds: NAME[I][J][K] (unused indices are 0); null ones are left out
//   end
// --summary prints, instead, the arena's size and its parts in MB (10^6 bytes):
//   echo width=3840 height=2160 levels=5 | session_plan_main --summary
#include <stdlib.h>

#include "session_plan.h"

using namespace ofx_plan;

static bool parse(char *line, ofx_params *p, SessionSwitches *sw)
{
    int fused = sw->iter_fused, pairs = sw->iter_pairs, dma = sw->iter_dma, pack = sw->pair_pack;
    struct Field {
        const char *name;
        int *at;
        int n;
    } fields[] = {{"width", &p->width, 1}, {"height", &p->height, 1}, {"levels", &p->levels, 1}, {"window", &p->window, 1}, {"mode", &p->mode, 1},
                  {"device", &p->device, 1}, {"sharded", &p->sharded, 1}, {"own_y0", p->own_y0, OFX_MAX_LEVELS}, {"own_y1", p->own_y1, OFX_MAX_LEVELS},
                  {"buf_y0", p->buf_y0, OFX_MAX_LEVELS}, {"buf_y1", p->buf_y1, OFX_MAX_LEVELS}, {"comp_y0", p->comp_y0, OFX_MAX_LEVELS},
                  {"comp_y1", p->comp_y1, OFX_MAX_LEVELS}, {"iters", &p->iters, 1}, {"local_corner", &p->local_corner, 1},
                  {"patch_size", &p->patch_size, 1}, {"stream_batch", &p->stream_batch, 1}, {"borrow_frames", &p->borrow_frames, 1},
                  {"stream_two_stage", &p->stream_two_stage, 1}, {"frames_partial", &p->frames_partial, 1}, {"deep_fetch", &p->deep_fetch, 1},
                  {"iter_fused", &fused, 1}, {"iter_pairs", &pairs, 1}, {"iter_dma", &dma, 1}, {"pair_pack", &pack, 1},
                  {"pair_waves", &sw->pair_waves, 1}, {"debug_corner_extent", &sw->debug_corner_extent, 1}};
    bool any = false;
    for (char *save = nullptr, *word = strtok_r(line, " \t\r\n", &save); word; word = strtok_r(nullptr, " \t\r\n", &save)) {
        char *eq = strchr(word, '=');
        const Field *f = nullptr;
        for (const Field &c : fields)
            if (eq && strlen(c.name) == (size_t)(eq - word) && !strncmp(c.name, word, (size_t)(eq - word))) f = &c;
        if (!eq || (!f && strncmp(word, "min_det=", 8))) {
            fprintf(stderr, "session_plan_main: what is '%s'?\n", word);
            exit(2);
        }
        any = true;
        if (!f) {
            p->min_det = (float)atof(eq + 1);
            continue;
        }
        const char *v = eq + 1;
        for (int i = 0; i < f->n && v; ++i) {
            f->at[i] = atoi(v);
            v = strchr(v, ',');
            if (v) ++v;
        }
    }
    sw->iter_fused = fused != 0, sw->iter_pairs = pairs != 0, sw->iter_dma = dma != 0, sw->pair_pack = pack != 0;
    return any;
}

static void print_plan(const SessionPlan &q)
{
    printf("plan B=%d n_sets=%d n_iter_sets=%d frames_per_slot=%d repair=%d debug_extent=%d fused_iters=%d iter_pairs=%d pair_pack=%d pair_waves=%d "
           "pscr_frame=%zu borrow_frames=%d stream_two_stage=%d total=%zu\n",
           q.B, q.n_sets, q.n_iter_sets, q.frames_per_slot, (int)q.repair, q.debug_extent, (int)q.fused_iters, (int)q.iter_pairs, q.pair_pack,
           q.pair_waves, q.pscr_frame, q.p.borrow_frames, q.p.stream_two_stage, q.total);
    for (int k = 0; k < q.p.levels; ++k) {
        const LevelPlan &l = q.lv[k];
        printf("level %d w=%d h=%d pitch=%d own0=%d own1=%d buf0=%d buf1=%d cmp0=%d cmp1=%d fl0=%d fl1=%d pw=%d ph=%d ppitch=%d plane_bytes=%zu "
               "flow_bytes=%zu patch_bytes=%zu\n",
               k, l.w, l.h, l.pitch, l.own0, l.own1, l.buf0, l.buf1, l.cmp0, l.cmp1, l.fl0, l.fl1, l.pw, l.ph, l.ppitch, l.plane_bytes, l.flow_bytes,
               l.patch_bytes);
    }
    auto at = [](const char *name, int i, int j, int k, size_t off) {
        if (off != kNoOffset) printf("at %s %d %d %d %zu\n", name, i, j, k, off);
    };
    const ArenaOffsets &o = q.off;
    for (int k = 0; k < OFX_MAX_LEVELS; ++k) {
        for (int t = 0; t < kSets; ++t) at("img", t, 0, k, o.img[t][k]), at("pimg", t, 0, k, o.pimg[t][k]);
        for (int t = 0; t < 2; ++t) at("sh", t, 0, k, o.sh[t][k]);
        for (int t = 0; t < kMaxBatch; ++t) {
            for (int j = 0; j < 3; ++j) at("itsh", t, j, k, o.itsh[t][j][k]);
            for (int f = 0; f < 2; ++f) at("pscr", t, f, k, o.pscr[t][f][k]);
            at("preloc", t, 0, k, o.preloc[t][k]);
            at("flowset", t, 0, k, o.flowset[t][k]);
            at("flowset2", t, 0, k, o.flowset2[t][k]);
        }
    }
    at("status", 0, 0, 0, o.status);
    at("uv", 0, 0, 0, o.uv);
    at("staging", 0, 0, 0, o.staging);
    printf("end\n");
}

static void print_summary(const SessionPlan &q)
{
    size_t planes = 0, flows = 0, patches = 0;
    for (int k = 0; k < q.p.levels; ++k) planes += q.lv[k].plane_bytes, flows += q.lv[k].flow_bytes, patches += q.lv[k].patch_bytes;
    const bool pimg = q.off.pimg[0][0] != kNoOffset, staging = q.off.staging != kNoOffset, flow2 = q.off.flowset2[0][0] != kNoOffset;
    const size_t tables = q.off.uv - q.off.status + align_up((size_t)OFX_MAX_LEVELS * 2 * sizeof(float) * kUvSlots, kAlign);
    struct {
        const char *what;
        size_t n, bytes;
    } parts[] = {{"image sets", (size_t)q.n_sets, planes},
                 {"shifted sets", 2, planes},
                 {"iteration scratch sets", (size_t)q.n_iter_sets, planes},
                 {"flow sets", (size_t)q.B, flows},
                 {"second flow sets", flow2 ? (size_t)q.B : 0, flows},
                 {"patch pyramids of the image sets", pimg ? (size_t)q.n_sets : 0, patches},
                 {"patch pyramids of the corner slots", (size_t)(q.frames_per_slot * q.B), q.pscr_frame},
                 {"status words and shift vectors", 1, tables},
                 {"3-channel staging frame", staging ? 1u : 0u, align_up((size_t)q.p.width * (size_t)q.p.height * 3, kAlign)}};
    size_t sum = 0;
    for (const auto &part : parts) {
        printf("%-36s %3zu x %10.3f MB = %10.3f MB\n", part.what, part.n, (double)part.bytes / 1e6, (double)(part.n * part.bytes) / 1e6);
        sum += part.n * part.bytes;
    }
    printf("%-36s %32.3f MB (%zu bytes)%s\n", "arena", (double)q.total / 1e6, q.total, sum == q.total ? "" : "  -- THE PARTS DO NOT ADD UP");
}

int main(int argc, char **argv)
{
    const bool summary = argc == 2 && !strcmp(argv[1], "--summary");
    if (argc > 2 || (argc == 2 && !summary)) {
        fprintf(stderr, "usage: %s [--summary] < descriptions\n", argv[0]);
        return 2;
    }
    static char line[4096];
    static SessionPlan plan;
    while (fgets(line, sizeof line, stdin)) {
        ofx_params p{};
        p.levels = 1, p.window = 9, p.mode = OFX_MODE_LK_FLOAT;
        SessionSwitches sw;
        if (!parse(line, &p, &sw)) continue;
        char err[512];
        const int rc = session_plan_make(&p, sw, &plan, err, sizeof err);
        if (rc != OFX_OK) printf("error %d %s\n", rc, err);
        else if (summary) print_summary(plan);
        else print_plan(plan);
    }
    return 0;
}
