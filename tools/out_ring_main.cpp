// The ring descriptor of the stream pipeline's output stages (csrc/out_ring.h) as a stand-alone host program: prints, for each
// (SLOTS, NEWEST, PAIR) triple on the command line, the slot index of the pair and whether the ring holds it.
// tests/test_out_ring.py builds and checks it.
//
//   out_ring_main SLOTS NEWEST PAIR [SLOTS NEWEST PAIR ...]
//
// Output: one line "SLOTS NEWEST PAIR INDEX HOLDS" per triple.  INDEX is printed for every pair >= 1, inside the window or not, and
// checked against the slot's address in a ring of 48-byte slots; it is "-" for a pair < 1: pairs count from 1, no caller asks for
// the slot of such a pair (holds() refuses it first), and (pair - 1) % slots is negative there in C++.
#include <stdio.h>
#include <stdlib.h>

#include "out_ring.h"

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: %s SLOTS NEWEST PAIR [SLOTS NEWEST PAIR ...]\n", argv[0]);
        return 2;
    }
    static char buffer[64 * 48];
    for (int i = 1; i < argc; i += 3) {
        const int slots = atoi(argv[i]);
        const long newest = atol(argv[i + 1]), pair = atol(argv[i + 2]);
        if (slots < 1 || slots > 64 || newest < 0) {
            fprintf(stderr, "%s: SLOTS 1 .. 64, NEWEST >= 0\n", argv[0]);
            return 2;
        }
        ofx_ring::OutRing r;
        r.set(buffer, 48, slots);
        r.newest = newest;
        if (!r.on()) return 1;
        if (pair < 1) {
            printf("%d %ld %ld - %d\n", slots, newest, pair, (int)r.holds(pair));
            continue;
        }
        if (r.slot(pair) != buffer + 48 * r.index(pair)) return 1;
        printf("%d %ld %ld %ld %d\n", slots, newest, pair, r.index(pair), (int)r.holds(pair));
    }
    ofx_ring::OutRing r;
    r.set(buffer, 48, 4);
    r.newest = 9;
    r.reset();
    return r.holds(9) || r.newest != 0 ? 1 : 0; // (a reset ring holds nothing)
}
