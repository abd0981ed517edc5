/* cc_poses.h — C-ABI of the per-firing odometry pose interpolation on gfx950.
 *
 * cc_engine_add_firings_device (cc_hip.h) reads three device arrays per call. The decoders (cc_kitti.h, cc_ouster.h, cc_velodyne.h,
 * cc_points.h) write two of them, d_xyz and d_intensity; this library writes the third, d_poses [streams][n][12] double, from
 * POSE TRACKS: per stream, a list of stamped odometry samples (odom_from_sensor, 3x4 row-major [R|t]) kept in device memory. A pose
 * between two samples is the reference loader's interpolation (kitti_loader.cpp:297-328, the host function cc_kitti_pose_interpolate):
 * std::lower_bound over the stamps; at or before the first sample and after the last one the raw sample, copied; otherwise the two
 * rotations as quaternions, slerp, back to a matrix, and the translations' lerp.
 *
 * Same operations in the same order as cc_kitti_pose_interpolate with ONE difference: slerp's acos and sin are not a libm's. They are
 * this project's own functions of IEEE + - * / sqrt (csrc/cc_pose_math.h), compiled once for the host and once for the device without
 * contraction. Hence: the device results equal the host twin below bit for bit, on every host; they equal cc_kitti_pose_interpolate
 * bit for bit where no acos / sin is involved (clamped poses, the linear branch of slerp, all translations and stamps) and to a few
 * units of 2^-53 in the rotation entries elsewhere. Parity with glibc's acos / sin is not attempted: glibc itself differs between CPUs.
 *
 * Functions return CC_OK (0) or a CC_ERR_* code of cc_hip.h; cc_poses_last_error() has the text (per thread).
 */
#ifndef CC_POSES_H
#define CC_POSES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_pose_tracks cc_pose_tracks;

const char* cc_poses_last_error(void);

/* ---- host twin (plain C, no device): what the kernels compute, on the CPU ------------------------------------------------------ */

/* stamps [n_samples] uint64 non-decreasing (not checked here), poses [n_samples][12]. out_poses [n_queries][12] = the pose at each of
 * query_stamps [n_queries]. n_samples >= 1, n_queries >= 0. */
int cc_poses_host_lookup(int64_t n_samples, const uint64_t* stamps, const double* poses, int64_t n_queries, const uint64_t* query_stamps,
                         double* out_poses);

/* The n firings of one sweep [start, end]: firing c has the stamp start + (uint64_t)((double)(end - start) * ((double)c / (n - 1)))
 * (cc_kitti_firing_stamps_and_poses, there with n = 2200). out_stamps [n] and out_poses [n][12]; either may be NULL. n < 2 and
 * end < start are refused. */
int cc_poses_host_sweep(int64_t n_samples, const uint64_t* stamps, const double* poses, int32_t n, uint64_t start, uint64_t end,
                        uint64_t* out_stamps, double* out_poses);

/* ---- device ------------------------------------------------------------------------------------------------------------------- */

/* One handle holds the tracks of num_streams streams, up to max_samples samples each. hip_stream: the hipStream_t every call is
 * enqueued on (pass cc_engine_hip_stream(e) and set the engine option "input_on_engine_stream" to chain with an engine; destroy the
 * handle before that engine); NULL = own stream. CC_ERR_NO_DEVICE without a gfx950 device: there is no CPU variant of this path. */
int cc_pose_tracks_create(cc_pose_tracks** out, int device, int num_streams, int max_samples, void* hip_stream);
void cc_pose_tracks_destroy(cc_pose_tracks* h);
void* cc_pose_tracks_hip_stream(cc_pose_tracks* h);
int cc_pose_tracks_sync(cc_pose_tracks* h);

/* Replace the track of `stream` by n samples from HOST arrays stamps [n], poses [n][12]. 1 <= n <= max_samples; stamps must not
 * decrease (equal neighbours are legal: the first of them is the one a query at that stamp meets, and nothing divides by their
 * difference). The arrays are copied before the call returns (through pinned staging of the handle); the upload is ordered on the
 * handle's stream, so calls enqueued earlier still see the old track and later ones the new. A live caller re-sets its recent window. */
int cc_pose_tracks_set(cc_pose_tracks* h, int stream, int n, const uint64_t* stamps, const double* poses);

/* One sweep per stream, all streams in one launch (asynchronous). HOST arrays h_start [S], h_end [S] and h_hold [S] (or NULL = all -1)
 * are copied before the call returns. Stream s:
 *   h_hold[s] == -1   d_poses[s][c] = the pose at the stamp of firing c of the sweep [h_start[s], h_end[s]], c in [0, n)
 *   h_hold[s] == k    0 <= k < samples of the track: d_poses[s][c] = raw sample k, verbatim, for every c (a stream that has ended and
 *                     is padded to keep it in step with the others)
 *   d_stamps[s][c]    (when d_stamps is not NULL) the stamp of firing c of the sweep, hold or not
 * DEVICE arrays: d_poses [S][n][12] double, 16-byte aligned; d_stamps [S][n] uint64 or NULL. Nothing outside [s][0 .. n) is touched.
 * CC_ERR_INVALID_ARGUMENT (nothing is launched) for n < 2, a NULL or misaligned d_poses, NULL h_start / h_end, h_end[s] < h_start[s],
 * a hold outside -1 .. samples - 1, a stream whose track was never set. */
int cc_pose_tracks_sweep(cc_pose_tracks* h, int n, const uint64_t* h_start, const uint64_t* h_end, const int32_t* h_hold, double* d_poses,
                         uint64_t* d_stamps);

/* The pose at each of n query stamps per stream, each written `repeat` times in a row (asynchronous):
 *   d_poses[s][q * repeat + r] = pose of stream s at d_query_stamps[s][q], r in [0, repeat)
 * repeat = columns per packet turns packet stamps into the per-firing poses of an Ouster packet (3 for a VLS-128 packet); repeat = 1
 * fills a decoder's d_packet_poses / d_message_poses. DEVICE arrays: d_query_stamps [S][n] uint64, d_poses [S][n * repeat][12] double,
 * 16-byte aligned. CC_ERR_INVALID_ARGUMENT (nothing is launched) for n < 1, repeat < 1, n * repeat beyond 31 bits, a NULL array, a
 * misaligned d_poses, a stream whose track was never set. */
int cc_pose_tracks_lookup(cc_pose_tracks* h, int n, const uint64_t* d_query_stamps, int repeat, double* d_poses);

#ifdef __cplusplus
}
#endif
#endif
