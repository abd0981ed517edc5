// Host-only probe of continuous_clustering_amd/csrc/cc_k_held.h for tests/test_held_range_cpu.py: the range a reader of held columns may look
// at, without HIP. Answers every "<first_column> <clear_done> <upper> <cursor> <ring_cols>" line from standard input with
// "range <from> <to> <lost> from <held_from>". No GPU.
#include <cinttypes>
#include <cstdio>

#define CC_HELD_RANGE_ONLY
#include "../../continuous_clustering_amd/csrc/cc_k_held.h"

int main()
{
    long long first = 0, cleared = 0, upper = 0, cursor = 0, ring = 0;
    while (scanf("%lld %lld %lld %lld %lld", &first, &cleared, &upper, &cursor, &ring) == 5)
    {
        const HeldRange r = held_range(first, cleared, upper, cursor, ring);
        printf("range %lld %lld %lld from %lld\n", r.from, r.to, r.lost, held_from(first, cleared, cursor));
    }
    return 0;
}
