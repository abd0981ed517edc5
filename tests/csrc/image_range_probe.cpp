// Host-only probe of continuous_clustering_amd/csrc/cc_k_held.h for tests/test_take_images_cpu.py: the range an image take writes, without
// HIP. Answers every "<first_column> <clear_done> <upper> <cursor> <ring_cols> <W> <slots>" line from standard input with
// "image <from> <to> <readable_from> <lost> <skipped> <rotation_from> <rotation_to> shares <rotation>:<written>:<lost> ...", one share per
// rotation the range touches (at most `slots`). No GPU.
#include <cinttypes>
#include <cstdio>

#define CC_HELD_RANGE_ONLY
#include "../../continuous_clustering_amd/csrc/cc_k_held.h"

int main()
{
    long long first = 0, cleared = 0, upper = 0, cursor = 0, ring = 0, W = 0, slots = 0;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld", &first, &cleared, &upper, &cursor, &ring, &W, &slots) == 7)
    {
        if (W < 1 || slots < 1)
            return 2;
        const ImageRange r = image_range(first, cleared, upper, cursor, ring, W, slots);
        printf("image %lld %lld %lld %lld %lld %lld %lld shares", r.from, r.to, r.readable_from, r.lost, r.skipped, r.rotation_from, r.rotation_to);
        long long rot = r.from / W;
        for (long long k = 0; k < slots && r.from < r.to && rot * W < r.to; k++, rot++)
        {
            long long written = 0, lost = 0;
            image_rotation_share(r, first, rot, W, &written, &lost);
            printf(" %lld:%lld:%lld", rot, written, lost);
        }
        printf("\n");
    }
    return 0;
}
