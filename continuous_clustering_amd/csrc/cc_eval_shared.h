// cc_eval_shared.h — what the two label compares share (kitti_evaluation.cpp:29-146): cc_eval_frame_device (cc_eval.hip, one frame per call) and
// the replay evaluator (cc_k_replay_eval.h / cc_replay_eval.h, the completed frames of all streams per call).
//   eval_point        device: one point's part of the ground confusion counts and of the contingency table between ground-truth
//                     euclidean-clustering labels and detection ids (lock-free atomicCAS hash table over the key gt << 32 | detection)
//   sum_entropies     host: OSE / USE from the exact pair counts, in the reference's order (ascending std::map keys, outer then inner) with the
//                     host's std::log — no floating-point reduction happens on the device
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/cc_hip.h"

namespace ccev
{

// semantic label ids of KittiLoader::getSemanticKittiLabelNameToLabelNumericMapping (kitti_loader.cpp:566-604) used by
// KittiEvaluation (kitti_evaluation.cpp:12-27)
constexpr uint16_t LABEL_UNLABELED = 0, LABEL_ROAD = 40, LABEL_PARKING = 44, LABEL_SIDEWALK = 48, LABEL_OTHER_GROUND = 49,
                   LABEL_LANE_MARKING = 60, LABEL_TERRAIN = 72;
constexpr unsigned long long EMPTY = ~0ull;

// point i of a frame of n points, called by every thread of a block of whole wavefronts (the ballots below need them all).
// counts5: tp, fn, fp, tn, and the pairs whose key looks like a free slot; keys / vals: the table, mask = its size - 1 (a power of two >= 2 n)
__device__ __forceinline__ void eval_point(const long long i, const long long n, const uint16_t* __restrict__ semantic,
                                           const uint32_t* __restrict__ euclid, const uint8_t* __restrict__ is_ground,
                                           const uint32_t* __restrict__ detection, unsigned long long* counts5, unsigned long long* keys,
                                           unsigned* vals, const unsigned mask)
{
    unsigned tp = 0, fn = 0, fp = 0, tn = 0;
    if (i < n)
    {
        const uint16_t sl = semantic[i];
        if (sl != LABEL_UNLABELED) // kitti_evaluation.cpp:49-50
        {
            const bool gt_ground = sl == LABEL_LANE_MARKING || sl == LABEL_ROAD || sl == LABEL_PARKING || sl == LABEL_SIDEWALK ||
                                   sl == LABEL_OTHER_GROUND || sl == LABEL_TERRAIN;
            const bool seg_ground = is_ground[i] != 0;
            tp = gt_ground && seg_ground;
            fn = gt_ground && !seg_ground;
            fp = !gt_ground && seg_ground;
            tn = !gt_ground && !seg_ground;
        }
        const uint32_t gt = euclid[i], det = detection[i];
        if (gt != 0 || det != 0) // points with neither label take part in no entropy term (kitti_evaluation.cpp:93-99)
        {
            const unsigned long long key = ((unsigned long long) gt << 32) | det;
            unsigned long long h = key * 0x9E3779B97F4A7C15ull;
            unsigned slot = (unsigned) (h >> 40) & mask;
            if (key == EMPTY) // (the one pair that looks like a free slot is counted beside the table)
                atomicAdd(&counts5[4], 1ull);
            else
            while (true)
            {
                const unsigned long long old = atomicCAS(&keys[slot], EMPTY, key);
                if (old == EMPTY || old == key)
                {
                    atomicAdd(&vals[slot], 1u);
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
    }
    // wave-level reduction of the four counters, one atomic per wave
    const unsigned long long m_tp = __ballot(tp), m_fn = __ballot(fn), m_fp = __ballot(fp), m_tn = __ballot(tn);
    if ((threadIdx.x & 63) == 0)
    {
        if (m_tp) atomicAdd(&counts5[0], (unsigned long long) __popcll(m_tp));
        if (m_fn) atomicAdd(&counts5[1], (unsigned long long) __popcll(m_fn));
        if (m_fp) atomicAdd(&counts5[2], (unsigned long long) __popcll(m_fp));
        if (m_tn) atomicAdd(&counts5[3], (unsigned long long) __popcll(m_tn));
    }
}

struct Pair
{
    uint32_t gt, det, n;
};

// the size of the table of a frame of n points: at least two slots per point, so that open addressing never meets a full table
inline unsigned table_size(const int64_t n)
{
    unsigned table = 1024;
    while ((int64_t) table < 2 * n)
        table <<= 1;
    return table;
}

// out->over_segmentation_entropy / under_segmentation_entropy from the frame's distinct (gt, det) pairs, in any order (sorted here)
inline void sum_entropies(std::vector<Pair>& pairs, cc_eval_frame_result* out)
{
    // over-segmentation entropy (kitti_evaluation.cpp:102-116): ground-truth clusters != 0 in ascending order, inside each the
    // detections (0 included) in ascending order
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.gt != b.gt ? a.gt < b.gt : a.det < b.det; });
    for (size_t i = 0; i < pairs.size();)
    {
        size_t j = i;
        unsigned long long total = 0;
        while (j < pairs.size() && pairs[j].gt == pairs[i].gt)
            total += pairs[j++].n;
        if (pairs[i].gt != 0)
            for (size_t k = i; k < j; k++)
            {
                const double frac = static_cast<double>(pairs[k].n) / static_cast<double>(total);
                out->over_segmentation_entropy -= frac * std::log(frac);
            }
        i = j;
    }
    // under-segmentation entropy (kitti_evaluation.cpp:125-145): detections != 0 ascending, inside each the ground-truth labels
    // (0 included) ascending; a detection that only contains ground truth 0 is skipped
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.det != b.det ? a.det < b.det : a.gt < b.gt; });
    for (size_t i = 0; i < pairs.size();)
    {
        size_t j = i;
        unsigned long long total = 0;
        while (j < pairs.size() && pairs[j].det == pairs[i].det)
            total += pairs[j++].n;
        const bool only_unlabeled = (j - i == 1) && pairs[i].gt == 0;
        if (pairs[i].det != 0 && !only_unlabeled)
            for (size_t k = i; k < j; k++)
            {
                const double frac = static_cast<double>(pairs[k].n) / static_cast<double>(total);
                out->under_segmentation_entropy -= frac * std::log(frac);
            }
        i = j;
    }
}

} // namespace ccev
