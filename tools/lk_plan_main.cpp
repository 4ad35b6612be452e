// What an LK launch does (csrc/lk_plan.h) as a stand-alone host program: prints the kernel variant and the strip table of a launch
// description.  tests/test_lk_plan.py builds and checks it; it is also how the figures in DESIGN.md section 4.5 were taken.
//
//   lk_plan_main NAME=VALUE ...          one description from the arguments
//   lk_plan_main < descriptions          one per line (a line without words is skipped)
//
//   launch=levels|tick                   an ofx_lk_levels launch or a stream tick's LK stage (default: tick)
//   mode=0|1|2 window=N sums=0|1         OFX_MODE_*; the window (default 9); levels: the inspection variant
//   accumulate=0|1 warp_out=0|1          of every item
//   hint=-1|0|1                          tick: ofx_stream_stages.deep_fetch
//   items=ITEM,ITEM,...                  ITEM = WxH[@Y0:Y1][/ROW0:ROW_END][pPITCH][fFLOW_ROW0]: a level, the rows the launch writes
//                                        (default all), the rows the planes hold (all), the pitch (W rounded up to 64), the flow
//                                        buffer's first row (0)
//   pyramid=WxH:LEVELS:PAIRS             appends the whole levels of PAIRS pairs, per pair the coarsest first (as a session's ticks do)
//   lk_dma= iter_dma= min_strip= waves_per_simd= fill= target_waves=      the switches OFX_LK_DMA ... (ofx_plan::LkSwitches)
//   out_w=N                              the tile's output width (TileGeom<R>::OUT_W: 248 up to 7x7, 240 up to 15x15, 232 up to 23x23, 224);
//                                        with it and a capacity the strips are printed
//   capacity=N | cus=N occ=N [reserve=N dflt=N full_fill=N]     the wave count planned for, or what it is computed from: the device's
//                                        CUs, the kernel's waves per SIMD and the call site's three numbers (default: the launch's)
//
// Output per description:
//   variant family=levels|iter|stream mode=M fast=F sums=S iter=I deep=D many=P      or: error CODE MESSAGE (and nothing more)
//   capacity N                                                                       (with cus and occ)
//   strips H=N waves=N                   the common strip height and the wave count, then per item
//   item I w=W h=H tiles_x=N strip_h=N first=N
//   end
//
//   lk_plan_main pyramid=3840x2160:5:8 out_w=240 cus=256 occ=5      (a 4K tick of 8 pairs, 9x9: strips of 90 rows, 4 096 waves)
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "lk_plan.h"

using namespace ofx_plan;

static void fail(const char *what, const char *word)
{
    fprintf(stderr, "lk_plan_main: %s '%s'\n", what, word);
    exit(2);
}

static LkItem parse_item(const char *word)
{
    LkItem a{};
    int used = 0;
    if (sscanf(word, "%dx%d%n", &a.w, &a.h, &used) != 2 || a.w <= 0 || a.h <= 0) fail("bad item", word);
    a.pitch = (a.w + 63) / 64 * 64, a.row_end = a.h, a.out_y1 = a.h;
    for (const char *p = word + used; *p; p += used) {
        used = 0;
        const bool ok = (*p == '@' && sscanf(p, "@%d:%d%n", &a.out_y0, &a.out_y1, &used) == 2) || (*p == '/' && sscanf(p, "/%d:%d%n", &a.row0, &a.row_end, &used) == 2) ||
                        (*p == 'p' && sscanf(p, "p%d%n", &a.pitch, &used) == 1) || (*p == 'f' && sscanf(p, "f%d%n", &a.flow_row0, &used) == 1);
        if (!ok || used == 0) fail("bad item", word);
    }
    if (a.out_y1 <= a.out_y0) fail("an item without rows", word);
    return a;
}

static void describe(char *line)
{
    std::string launch = "tick";
    int mode = OFX_MODE_LK_FLOAT, window = 9, sums = 0, accumulate = 0, warp_out = 0, hint = 0, out_w = 0, capacity = 0, cus = 0, occ = 0, reserve = -1, dflt = -1,
        full_fill = kLkFullFill;
    LkSwitches sw;
    std::vector<LkItem> items;
    struct {
        const char *name;
        int *at;
    } fields[] = {{"mode", &mode}, {"window", &window}, {"sums", &sums}, {"accumulate", &accumulate}, {"warp_out", &warp_out}, {"hint", &hint}, {"out_w", &out_w},
                  {"capacity", &capacity}, {"cus", &cus}, {"occ", &occ}, {"reserve", &reserve}, {"dflt", &dflt}, {"full_fill", &full_fill}, {"lk_dma", &sw.lk_dma},
                  {"iter_dma", &sw.iter_dma}, {"min_strip", &sw.min_strip}, {"waves_per_simd", &sw.waves_per_simd}, {"fill", &sw.fill}, {"target_waves", &sw.target_waves}};
    bool any = false;
    for (char *save = nullptr, *word = strtok_r(line, " \t\r\n", &save); word; word = strtok_r(nullptr, " \t\r\n", &save)) {
        char *eq = strchr(word, '=');
        if (!eq) fail("what is", word);
        const std::string name(word, eq - word);
        any = true;
        if (name == "launch") {
            launch = eq + 1;
        } else if (name == "items") {
            for (char *s2 = nullptr, *it = strtok_r(eq + 1, ",", &s2); it; it = strtok_r(nullptr, ",", &s2)) items.push_back(parse_item(it));
        } else if (name == "pyramid") {
            int w, h, levels, pairs;
            if (sscanf(eq + 1, "%dx%d:%d:%d", &w, &h, &levels, &pairs) != 4 || levels < 1 || (w >> (levels - 1)) < 1 || (h >> (levels - 1)) < 1) fail("bad pyramid", word);
            for (int p = 0; p < pairs; ++p)
                for (int k = levels - 1; k >= 0; --k) items.push_back(parse_item((std::to_string(w >> k) + "x" + std::to_string(h >> k)).c_str()));
        } else {
            bool known = false;
            for (const auto &f : fields)
                if (name == f.name) *f.at = atoi(eq + 1), known = true;
            if (!known) fail("what is", word);
        }
    }
    if (!any) return;
    if (launch != "tick" && launch != "levels") fail("what launch is", launch.c_str());
    if (items.size() > OFX_MAX_LK_ITEMS) fail("too many items in", launch.c_str());
    if (sw.min_strip < 1) fail("min_strip must be >= 1 in", launch.c_str());
    for (LkItem &a : items) a.accumulate = accumulate, a.warp_out = warp_out;
    const int n = (int)items.size();
    LkVariant v{};
    if (launch == "tick") {
        v = lk_tick_variant(items.data(), n, mode, hint, sw);
    } else if (n > 0) {
        char err[160];
        const int rc = lk_levels_variant(items.data(), n, window >> 1, mode, sums != 0, sw, &v, err, sizeof err);
        if (rc != OFX_OK) {
            printf("error %d %s\n", rc, err);
            return;
        }
    }
    if (n > 0 || launch == "tick")
        printf("variant family=%s mode=%d fast=%d sums=%d iter=%d deep=%d many=%d\n", v.family == kLkLevels ? "levels" : v.family == kLkIter ? "iter" : "stream", v.mode,
               (int)v.fast, (int)v.sums, v.iter, (int)v.deep, (int)v.many);
    if (cus > 0 && occ > 0) {
        const bool tick = launch == "tick";
        capacity = lk_wave_capacity(cus, occ, reserve >= 0 ? reserve : (tick ? kTickReserve : 0), dflt >= 0 ? dflt : (tick ? tick_waves_per_simd(v.many) : kLkWavesPerSimd),
                                    full_fill, sw);
        printf("capacity %d\n", capacity);
    }
    if (n > 0 && out_w > 0 && capacity > 0) {
        static LkStrips s;
        lk_strips(items.data(), n, out_w, sw.min_strip, capacity, &s);
        printf("strips H=%d waves=%d\n", s.H, s.blocks);
        for (int i = 0; i < n; ++i) printf("item %d w=%d h=%d tiles_x=%d strip_h=%d first=%d\n", i, items[i].w, items[i].h, s.tiles_x[i], s.strip_h[i], s.first_block[i]);
    }
    printf("end\n");
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        std::string line;
        for (int i = 1; i < argc; ++i) line += std::string(argv[i]) + " ";
        describe(&line[0]);
        return 0;
    }
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) describe(line);
    return 0;
}
