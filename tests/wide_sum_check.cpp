// Host check of csrc/wide_sum.h, driven by tests/test_wide_sum.py: reads one request per line from stdin and answers it on stdout.
//   c HI LO          the float64 nearest to the signed 128-bit integer (LO, HI), as the 16 hex digits of its bits
//   a HI LO AHI ALO  (LO, HI) += (ALO, AHI) through wide_add, as "HI LO"
// All numbers are 64-bit hex.  Ends with "ok N" after N requests.
#include <stdio.h>
#include <string.h>

#include "wide_sum.h"

int main()
{
    char op;
    long n = 0;
    while (scanf(" %c", &op) == 1) {
        wide_u64 hi, lo, ahi, alo;
        if (op == 'c') {
            if (scanf("%llx %llx", &hi, &lo) != 2) return 2;
            const double d = wide_to_double(lo, hi);
            wide_u64 bits;
            memcpy(&bits, &d, sizeof bits);
            printf("%016llx\n", bits);
        } else if (op == 'a') {
            if (scanf("%llx %llx %llx %llx", &hi, &lo, &ahi, &alo) != 4) return 2;
            wide_add(lo, hi, alo, ahi);
            printf("%016llx %016llx\n", hi, lo);
        } else {
            return 2;
        }
        ++n;
    }
    printf("ok %ld\n", n);
    return 0;
}
