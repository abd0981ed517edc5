/* cc_kitti.h — C-ABI of the KITTI replay path that sits immediately upstream of insertion.
 *
 * The reference turns one KITTI / SemanticKITTI velodyne frame (an unorganised, ego-motion-corrected cloud in a .bin
 * file) into 2200 pseudo-firings of 64 lasers that it feeds to ContinuousClustering::addFiring
 * (src/tools/kitti_demo.cpp:352-395). The per-point steps of that conversion are KittiLoader methods
 * (src/evaluation/kitti_loader.cpp):
 *
 *     recoverLaserIndices      :48-99    row of every point from the azimuth jumps of the file order
 *     undoEgoMotionCorrection  :177-210  per-point rigid transform picked from a 1-ms bin table
 *     generateRangeImage       :101-175  azimuth binning into 64 x 2200 cells with the shift-if-occupied rule
 *     makePseudoFiringFromRangeImageColumn  kitti_demo.cpp:123-159  one firing per range-image column
 *
 * This library runs them as HIP kernels on gfx950 and leaves the firings in HBM in exactly the layout
 * cc_engine_add_firings_device (cc_hip.h) consumes, so a replayed frame never returns to the host between the .bin
 * upload and the published columns. The small per-frame / per-firing pose arithmetic of the same call sites (slerp between
 * two poses, the bin table) is host code behind the same ABI. There is no CPU variant of the per-point steps.
 *
 * All poses are 3x4 row-major [R|t] doubles (12 values), stamps are nanoseconds. Functions return CC_OK (0) or a CC_ERR_*
 * code of cc_hip.h; cc_kitti_last_error() has the text.
 */
#ifndef CC_KITTI_H
#define CC_KITTI_H

#include <stdint.h>

#include "cc_hip.h" /* cc_eval_frame_result, the CC_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* KittiLoader::RANGE_IMAGE_HEIGHT / RANGE_IMAGE_WIDTH (kitti_loader.hpp:84-86) */
#define CC_KITTI_ROWS 64
#define CC_KITTI_COLS 2200

typedef struct cc_kitti cc_kitti;

/* which steps one cc_kitti_convert_frames call runs for a frame */
enum
{
    CC_KITTI_RECOVER_ROWS = 1,    /* recoverLaserIndices; without it the rows come from cc_kitti_frame::laser_index */
    CC_KITTI_UNDO_EGO_MOTION = 2, /* undoEgoMotionCorrection with cc_kitti_frame::bin_transforms */
    CC_KITTI_RANGE_IMAGE = 4,     /* generateRangeImage */
    CC_KITTI_SHIFT_OCCUPIED = 8,  /* its shift_cell_if_already_occupied argument (default true in the reference) */
    CC_KITTI_FIRINGS = 16         /* makePseudoFiringFromRangeImageColumn for all 2200 columns (needs RANGE_IMAGE) */
};
#define CC_KITTI_ALL_STAGES 31u

typedef struct cc_kitti_frame
{
    const float* points;        /* n_points x 4 floats (x, y, z, i) — the .bin payload (loadPointCloud, kitti_loader.cpp:12-29); host */
    int64_t n_points;
    const uint8_t* laser_index; /* host, n_points; read when CC_KITTI_RECOVER_ROWS is not set (NULL = all rows 0) */
    uint32_t stages;
    int32_t num_bins;                /* rows of bin_transforms */
    uint64_t rotation_start_stamp;   /* undoEgoMotionCorrection arguments */
    uint64_t rotation_end_stamp;
    const double* bin_transforms;    /* host, num_bins x 12: velodyne_from_velodyne of every 1-ms bin (cc_kitti_bin_transforms) */
    /* CC_KITTI_FIRINGS outputs, DEVICE pointers (NULL = not wanted): */
    float* d_xyz;              /* [2200][64][3] RawPoint::x,y,z of firing c, laser r (NaN = empty cell) */
    uint8_t* d_intensity;      /* [2200][64]    static_cast<uint8_t>(i * 255), 0 for empty cells */
    int32_t* d_original_index; /* [2200][64]    KittiPoint::original_kitti_index, -1 for empty cells */
} cc_kitti_frame;

typedef struct cc_kitti_frame_info
{
    int32_t rows_found;   /* laser_index + 1 at the end of recoverLaserIndices (kitti_loader.cpp:92); 64 for a healthy frame */
    int32_t max_columns;  /* its max_columns statistic (:80); the reference throws when it exceeds 2200 (:96-97) */
    int64_t break_index;  /* first point of the 65th row (:74-76), n_points if there is none; points from here on keep row 0 */
    int64_t skipped;      /* points whose azimuth is NaN (the reference indexes out of bounds for them; they are left out) */
} cc_kitti_frame_info;

/* max_frames: frames one cc_kitti_convert_frames call may carry (each gets a device slot); max_points: per frame.
 * hip_stream: the hipStream_t everything is enqueued on (pass cc_engine_hip_stream(e) to chain with an engine); NULL = own stream. */
int cc_kitti_create(cc_kitti** out, int device, int max_frames, int64_t max_points, void* hip_stream);
void cc_kitti_destroy(cc_kitti* k);
const char* cc_kitti_last_error(void);

/* Upload the frames (slot i = frames[i]) and enqueue their stages. Returns without synchronising. */
int cc_kitti_convert_frames(cc_kitti* k, int n_frames, const cc_kitti_frame* frames);
int cc_kitti_sync(cc_kitti* k);
void* cc_kitti_hip_stream(cc_kitti* k);

/* Results of slot `slot` of the last cc_kitti_convert_frames call (synchronises). Any pointer may be NULL.
 *   h_points       n_points x 4: the points after undoEgoMotionCorrection (or as uploaded)
 *   h_laser_index  n_points
 *   h_cell_source  [64][2200] (row-major like the reference's organized_points, kitti_loader.cpp:165): the original index of the
 *                  point that generateRangeImage leaves in each cell, -1 for an empty cell */
int cc_kitti_frame_result(cc_kitti* k, int slot, cc_kitti_frame_info* info, float* h_points, uint8_t* h_laser_index,
                          int32_t* h_cell_source);

/* ---- the frame scatter of the harness, addColumnAndEvaluateFrameIfCompleted (kitti_demo.cpp:173-224), on the device --------------------
 * For an engine whose streams are each fed exactly num_columns pseudo-firings per frame (kitti_demo.cpp:386-403; cc_kitti_convert_frames
 * writes them straight into the engine's input arrays). A published cell then names its KITTI point through the sequence number of the
 * firing that filled it: frame = sequence / num_columns, column of the frame = sequence % num_columns, point =
 * d_original_index[stream][frame % slots][column][row] (cc_kitti_frame::d_original_index of that frame's conversion; `slots` frames are
 * kept per stream, 4 are enough: a column is published within a rotation of its insertion).
 *   cc_engine_scatter_info   per published column of the ranges [from[i], to[i]] of streams[i] (concatenated in the outputs): the smallest
 *                            and largest frame index among the column's points (INT32_MAX / -1 for a column without points) — what the
 *                            harness needs to find the column in which frame N + 1 starts (:205-209) and its two error cases (:203-206).
 *   cc_engine_scatter_apply  is_ground_point = (ground_point_label == GP_GROUND) and detection_label = id (:214-215) of the points of the
 *                            columns [from, to] into d_is_ground / d_detection, laid out [stream][frame % slots][max_points]; asynchronous
 *                            on cc_engine_hip_stream(e). cc_eval_frame_device (cc_hip.h) evaluates a frame from those arrays.
 * Both are declared here because they belong to the replay harness; they live in the engine (include cc_hip.h first). */
struct cc_engine;
int cc_engine_scatter_info(struct cc_engine* e, int n, const int32_t* streams, const int64_t* from, const int64_t* to,
                           const int32_t* d_original_index, int slots, int32_t* h_min_frame, int32_t* h_max_frame);
int cc_engine_scatter_apply(struct cc_engine* e, int stream, int64_t from, int64_t to, const int32_t* d_original_index, int slots,
                            uint8_t* d_is_ground, uint32_t* d_detection, int64_t max_points);

/* ---- the same scatter plus the evaluation of the frames it completes, for all streams in one call ----------------------------------------
 * A replay evaluator is bound to an engine whose streams are fed as above. Per cc_replay_eval_step it takes, for every active stream, the
 * columns published since the last step (one cursor per stream in device memory, as cc_engine_take_points has them), finds where frames
 * complete, writes is_ground / detection of the columns' points into the frames' arrays, evaluates every completed frame
 * (kitti_evaluation.cpp:29-146) and returns one record per frame. The records are bit-equal to cc_engine_scatter_info / _apply +
 * cc_eval_frame_device driven by the host walk: the integer work runs on the device, the entropies are summed on the host from the exact pair
 * counts in std::map order with the host's std::log (the code cc_eval_frame_device uses).
 *
 * Storage (device memory, owned by the handle, allocated by cc_replay_eval_create; nothing is allocated or freed afterwards):
 *   original_index [streams][slots][num_columns][num_rows], initialised to -1; semantic, euclid, is_ground, detection
 *   [streams][slots][max_points]; n_points [streams][slots]; (cursor, previous_frame, active) per stream, cursor and previous_frame starting
 *   at 0, active at 1; `eval_lanes` evaluation workspaces (a hash table of the power of two >= 2 * max_points slots each, cc_eval_frame_device's
 *   rule). Frame f of a stream uses slot f % slots.
 * The caller's rule for `slots`: slots >= frames fed between two steps + 3 (a column is published within a rotation of its insertion, so the
 * frames previous_frame .. previous_frame + 2 + frames fed are alive at a step). At most `slots` frames of a stream complete per step; a stream
 * that has more goes on in the next step.
 *
 * cc_replay_eval_original_index  where the converter writes cc_kitti_frame::d_original_index of frame `frame` of `stream`.
 * cc_replay_eval_add_frame       the ground truth of a frame (host arrays of n_points entries) into its slot, the slot's is_ground / detection to
 *                                zero; enqueued on cc_engine_hip_stream(e) through pinned staging of the handle, no synchronisation of its own
 *                                (it waits only if all of the handle's staging blocks, one per stream, are still in flight).
 *                                CC_ERR_INVALID_ARGUMENT: n_points > max_points; frame >= previous_frame + slots (that slot still belongs to a
 *                                frame that has not been evaluated); frame < 0.
 * cc_replay_eval_set_active      an inactive stream is not walked (a sequence without labels, a stream that has finished).
 * cc_replay_eval_seek            sets the cursor and previous_frame of one stream and clears its CC_REPLAY_ERR_*. After cc_engine_reset_streams
 *                                on a stream that starts another sequence: seek(stream, 0, 0).
 * cc_replay_eval_step            finishes the submitted batches first. Walks, per active stream without an error, the columns
 *                                [max(cursor, clear_done, first column), first_unpublished) as addColumnAndEvaluateFrameIfCompleted does: only
 *                                cells that hold a return and whose original_index is >= 0 count; a segment ends with the first column whose
 *                                largest frame is previous_frame + 1, then frame previous_frame is complete and previous_frame increments. A
 *                                segment with a column whose smallest frame is < previous_frame raises CC_REPLAY_ERR_ALREADY_EVALUATED, one
 *                                with a column whose largest frame is > previous_frame + 1 CC_REPLAY_ERR_TOO_FAR_AHEAD (the reference's two
 *                                runtime_errors, kitti_demo.cpp:203-206): that segment is not applied, the cursor stays at its first column
 *                                (error_column), frames completed by earlier segments of the step are still delivered, the stream reports the
 *                                error in every step until cc_replay_eval_seek, other streams are unaffected. Columns already cleared are
 *                                counted in lost_columns and read as empty. finish[s] != 0 additionally evaluates previous_frame of stream s
 *                                with what has been published by now (kitti_demo.cpp:417-419) and makes the stream inactive (ignored for a
 *                                stream that is inactive or has an error). Records are ordered by stream, then frame. If they exceed `capacity`:
 *                                CC_ERR_CAPACITY, *n_records and h_table[].frames_evaluated say what is needed, nothing is applied or evaluated,
 *                                no cursor and no previous_frame moves (h_table[].previous_frame is the unchanged one), and a retry with room
 *                                returns what a first call would have. More completed frames than eval_lanes are evaluated in
 *                                ceil(frames / eval_lanes) rounds inside the call. Refused (CC_ERR_INVALID_ARGUMENT) while the option "resident"
 *                                is on. Returns synchronised.
 * cc_replay_eval_counters        kernel launches and host synchronisations of the steps so far, beyond what finishing the submitted batches
 *                                takes. Per step, with L = the longest column range of the plan and R = eval_rounds of the step:
 *                                    kernel_launches = 3 + (L > 0 ? 2 : 0) + 2 R      (plan, [info], walk, scan, [apply], R x (eval, compact))
 *                                    host_syncs      = 2 + R                          (after the plan, after the scan, one per round)
 *                                Neither depends on the number of streams. A step that returns CC_ERR_CAPACITY has R = 0.
 * Destroy the evaluator before its engine. */
#define CC_REPLAY_ERR_ALREADY_EVALUATED 101 /* "Found a point belonging to a frame that was already evaluated!" */
#define CC_REPLAY_ERR_TOO_FAR_AHEAD 102     /* "Found a point whose frame is too far ahead!" */

typedef struct cc_replay_eval cc_replay_eval;
typedef struct cc_replay_record
{
    int32_t stream, frame;
    cc_eval_frame_result r;
} cc_replay_record; /* 56 bytes */
typedef struct cc_replay_stream /* one per stream */
{
    int64_t col_from, col_to;   /* columns [col_from, col_to) were scattered in this step */
    int64_t lost_columns;       /* columns between the cursor and what had been cleared already */
    int64_t error_column;       /* first column of the segment that raised `error`, else -1 */
    int32_t previous_frame;     /* after the step (kitti_demo.cpp previous_frame_index) */
    int32_t frames_evaluated;   /* records of this stream in this step */
    int32_t error;              /* 0, CC_REPLAY_ERR_ALREADY_EVALUATED, CC_REPLAY_ERR_TOO_FAR_AHEAD, or the stream's CC_ERR_* */
    int32_t active;
} cc_replay_stream;

int cc_replay_eval_create(cc_replay_eval** out, struct cc_engine* e, int slots, int64_t max_points, int eval_lanes);
void cc_replay_eval_destroy(cc_replay_eval* h);
int32_t* cc_replay_eval_original_index(cc_replay_eval* h, int stream, int64_t frame);
int cc_replay_eval_add_frame(cc_replay_eval* h, int stream, int64_t frame, int64_t n_points, const uint16_t* semantic, const uint32_t* euclid);
int cc_replay_eval_set_active(cc_replay_eval* h, int stream, int active);
int cc_replay_eval_seek(cc_replay_eval* h, int stream, int64_t column, int32_t previous_frame);
int cc_replay_eval_step(cc_replay_eval* h, const uint8_t* finish, cc_replay_record* records, int64_t capacity, int64_t* n_records,
                        cc_replay_stream* h_table);
int cc_replay_eval_counters(cc_replay_eval* h, uint64_t* steps, uint64_t* kernel_launches, uint64_t* host_syncs, uint64_t* eval_rounds);
/* Test entry: evaluates the frames `frames[i]` of stream `stream` from their slots as they are (no walk, no apply, no cursor moves), in rounds
 * of eval_lanes, and writes n records. What tests of the batched label compare alone drive, after cc_replay_eval_add_frame and writes to
 * cc_replay_eval_slot_arrays. Its rounds count like a step's (two launches, one synchronisation, one eval_round each); `steps` stays. */
int cc_replay_eval_evaluate_slots(cc_replay_eval* h, int stream, int n, const int32_t* frames, cc_replay_record* records);
/* Device pointers of the slot of frame `frame` of `stream`: is_ground (uint8) and detection (uint32), max_points entries each. */
int cc_replay_eval_slot_arrays(cc_replay_eval* h, int stream, int64_t frame, uint8_t** d_is_ground, uint32_t** d_detection);

/* ---- host-side pose arithmetic of the same call sites (plain C, no device work) ------------------------------------------ */

/* KittiLoader::interpolate (kitti_loader.cpp:297-328): pose at `stamp` from stamp-sorted poses (slerp + lerp, clamped at the ends). */
int cc_kitti_pose_interpolate(int64_t n_poses, const uint64_t* stamps, const double* poses, uint64_t stamp, double out[12]);
/* The lookup table of undoEgoMotionCorrection (kitti_loader.cpp:183-197). Writes num_bins x 12 doubles to `out` (capacity in
 * bins) and returns num_bins through *num_bins. */
int cc_kitti_bin_transforms(int64_t n_poses, const uint64_t* stamps, const double* poses, uint64_t rotation_start_stamp,
                            uint64_t rotation_end_stamp, const double mid_pose[12], double* out, int32_t capacity, int32_t* num_bins);
/* Stamp (kitti_demo.cpp:132-135) and interpolated odom_from_velodyne (kitti_demo.cpp:388-389) of the 2200 pseudo-firings of a frame. */
int cc_kitti_firing_stamps_and_poses(int64_t n_poses, const uint64_t* stamps, const double* poses, uint64_t start_stamp,
                                     uint64_t end_stamp, uint64_t* out_stamps, double* out_poses);
/* KittiLoader::getStartEndTimestampsVelodyne (kitti_loader.cpp:525-540). */
int cc_kitti_start_end_stamps(int64_t n, const uint64_t* middle, uint64_t* start, uint64_t* end);
/* One line of poses.txt -> odom_from_x (getAllDynamicTransforms, kitti_loader.cpp:330-369): odom_from_first_cam0 * first_cam0_from_cam0 *
 * cam0_from_x, where row12 are the 12 numbers of the line. */
int cc_kitti_pose_from_line(const double row12[12], const double cam0_from_x[12], double out[12]);

#ifdef __cplusplus
}
#endif
#endif
