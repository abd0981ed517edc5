/* cc_stamps.h — C-ABI of the firing-stamp log on gfx950: the time stamps of what the takes of cc_hip.h hand over, resolved
 * in device memory.
 *
 * Every message of the reference carries a stamp derived from point stamps: the cluster callback's stamp_cluster (cc.cpp:1007-1010,
 * 1025-1028), the header stamp of a column cloud (ros_utils.cpp:51-71), the time_sec / time_nsec fields of a point (ros_utils.cpp:251-266).
 * The engine does not carry stamps; a record of cc_engine_take_points / cc_engine_take_clusters carries cc_take_point::source_firing, the
 * low 32 bits of the index of the firing it came from. This library keeps the stamps of the recent firings of every stream in device
 * memory, keyed by that index, and turns the records of a take into stamps without a host round trip.
 *
 * ONE STAMP PER FIRING. Every front end of the reference gives all rows of a firing the same stamp (ouster_input.hpp:165;
 * velodyne_input.hpp:57-58, whose per-point offset is always 0; generic_points_input.hpp:38-41; the KITTI loader's per-firing stamps), so a
 * firing has one stamp here, uint64 nanoseconds.
 *
 * THE LOG. cc_firing_stamps holds, per stream, a ring of `capacity` stamps (a power of two) and a 64-bit `head`: the index the next pushed
 * firing gets. It counts as the engine's source_firing counts: every firing passed to cc_engine_add_firings(_device), all-NaN placeholder
 * firings included, from 0 after a reset. Push what you add to the engine, in the same order; reset what you reset. An engine stream whose
 * `error` is set is skipped by the engine while the log still advances: such a stream hands over nothing until it is reset, and the caller
 * resets both, so the two counts meet again at 0.
 *
 * RESOLUTION of a record with the low bits f (csrc/cc_stamp_math.h, one text for kernels and host twins): with head == 0, or with nothing
 * pushed since the last seek, the firing is missing; otherwise last = head - 1 and idx = last - (uint32_t)((uint32_t)last - f), the newest
 * pushed firing with those low bits; it is missing if last - idx >= capacity or if idx lies below what a seek forgot; otherwise its stamp is
 * ring[idx & (capacity - 1)]. A missing firing resolves to stamp 0 and is counted (cc_firing_stamps_counters; every resolve call below
 * counts the records it resolves). Stamp 0 is also what the reference holds in a cell it has no stamp for (cc.cpp:1121); it skips stamp 0
 * in column headers (ros_utils.cpp:65) and does not skip it in a cluster's min / max. Both are reproduced.
 *
 * Everything is integer arithmetic: the device results equal the host twins bit for bit and do not depend on the launch shape.
 * Functions return CC_OK (0) or a CC_ERR_* code of cc_hip.h; cc_firing_stamps_last_error() has the text (per thread).
 */
#ifndef CC_STAMPS_H
#define CC_STAMPS_H

#include <stdint.h>

#include "cc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_firing_stamps cc_firing_stamps;

typedef struct cc_cluster_stamp {   /* 32 bytes, one per cluster of a cc_engine_take_clusters */
    uint64_t stamp;                 /* use_last_point ? max_stamp : min_stamp + (max_stamp - min_stamp) / 2   (cc.cpp:1025-1028) */
    uint64_t min_stamp, max_stamp;  /* over ALL members, zeros (missing firings) included, unsigned compares (cc.cpp:1007-1010) */
    uint32_t n_missing;             /* members whose firing was not in the log */
    uint32_t pad;
} cc_cluster_stamp;

const char* cc_firing_stamps_last_error(void);

/* ---- host twins (plain C, no device): what the kernels compute, on the CPU ------------------------------------------------------ */

/* `capacity` rounded up to a power of two (at least 1); 0 when capacity < 1 or the result would exceed 2^31. */
int64_t cc_stamps_round_capacity(int64_t capacity);

typedef struct cc_stamps_host_log { /* the log of num_streams streams in host memory */
    int32_t num_streams, pad;
    int64_t capacity;               /* a power of two */
    uint64_t* rings;                /* [num_streams][capacity] */
    uint64_t* heads;                /* [num_streams] */
    uint64_t* floors;               /* [num_streams]: firings below are forgotten (0, or where a seek put the head) */
    uint64_t* missing;              /* [num_streams]: the resolve twins add to it */
} cc_stamps_host_log;

/* Stream `stream` (-1: every stream, stamps is [num_streams][n] then) advances by n * repeat firings, each stamp written `repeat` times. */
int cc_stamps_host_push(cc_stamps_host_log* log, int stream, int64_t n, const uint64_t* stamps, int repeat);
/* stamps [n] and missing [n] (uint8, may be NULL) of the low-32-bit keys firings [n] of `stream`; counts nothing. */
int cc_stamps_host_resolve(const cc_stamps_host_log* log, int stream, int64_t n, const uint32_t* firings, uint64_t* stamps, uint8_t* missing);
/* out [n][2] = seconds (truncated to 32 bits), nanoseconds of stamps [n] (ros::Time::fromNSec). */
int cc_stamps_host_sec_nsec(int64_t n, const uint64_t* stamps, uint32_t* out);
/* The three resolve calls below over HOST arrays; same arguments, same results, same counting. */
int cc_stamps_host_of_points(cc_stamps_host_log* log, int64_t n_records, const cc_take_point* records, const cc_take_stream* table,
                             uint64_t* stamps, uint32_t* sec_nsec);
int cc_stamps_host_of_columns(cc_stamps_host_log* log, int64_t n_records, const cc_take_point* records, const cc_take_stream* table,
                              uint64_t* column_stamps, uint64_t* stream_stamps);
int cc_stamps_host_of_clusters(cc_stamps_host_log* log, int use_last_point, int64_t n_clusters, const cc_take_cluster* clusters,
                               int64_t n_records, const cc_take_point* records, cc_cluster_stamp* out, uint64_t* point_stamps);

/* ---- device ------------------------------------------------------------------------------------------------------------------- */

/* `capacity` firings per stream are kept (rounded up to a power of two, at most 2^31; num_streams at most 65535). Rule of thumb: at least
 * the firings of the engine ring's columns plus those of one call, so that whatever a take can still hand over is still held.
 * hip_stream: the hipStream_t every call is enqueued on (pass cc_engine_hip_stream(e) to chain with an engine; destroy the handle before
 * that engine); NULL = own stream. CC_ERR_NO_DEVICE without a gfx950 device: there is no CPU variant of this path. */
int cc_firing_stamps_create(cc_firing_stamps** out, int device, int num_streams, int64_t capacity, void* hip_stream);
void cc_firing_stamps_destroy(cc_firing_stamps* h);
void* cc_firing_stamps_hip_stream(cc_firing_stamps* h);
int cc_firing_stamps_sync(cc_firing_stamps* h);
int64_t cc_firing_stamps_capacity(cc_firing_stamps* h);   /* the rounded capacity; 0 for a NULL handle */

/* DEVICE array d_stamps [S][n] uint64, 8-byte aligned: every stream advances by n * repeat firings, each stamp written `repeat` times in a
 * row (repeat = columns per packet for packet stamps, 1 for the d_stamps of cc_pose_tracks_sweep: the convention of cc_pose_tracks_lookup).
 * Asynchronous on the handle's stream; d_stamps must stay unchanged until the call has run. Refused: n < 1, repeat < 1,
 * n * repeat > capacity, a NULL or misaligned d_stamps. */
int cc_firing_stamps_push(cc_firing_stamps* h, int64_t n, const uint64_t* d_stamps, int repeat);
/* For callers of the single-stream cc_engine_add_firings: HOST array stamps [n], copied before the call returns; `stream` advances by n
 * firings (1 <= n <= capacity). */
int cc_firing_stamps_push_host(cc_firing_stamps* h, int stream, int64_t n, const uint64_t* stamps);
/* head = next_firing and nothing held: for attaching to an engine whose stream has consumed firings already. */
int cc_firing_stamps_seek(cc_firing_stamps* h, int stream, uint64_t next_firing);
/* head = 0, nothing held, missing = 0 for each of streams [n]; call it with cc_engine_reset_streams / cc_engine_reset. n == 0 does nothing. */
int cc_firing_stamps_reset_streams(cc_firing_stamps* h, int n, const int* streams);
/* Synchronises. *head of `stream` and *missing, the records resolved so far (since create or the stream's reset) whose firing was not in
 * the log; either may be NULL. */
int cc_firing_stamps_counters(cc_firing_stamps* h, int stream, uint64_t* head, uint64_t* missing);

/* The three resolve calls. All arrays are DEVICE arrays unless named h_; all are asynchronous on the handle's stream, ordered behind earlier
 * pushes, and read the output of a take that has returned (a take returns with its output complete). Records: 16-byte aligned, as the takes
 * require; outputs 8-byte aligned (d_out 16). Zero records or clusters is legal, launches nothing and returns CC_OK. Refusals
 * (CC_ERR_INVALID_ARGUMENT) launch nothing.
 *
 * _of_points: d_stamps[i] = the stamp of record i of a cc_engine_take_points; d_table is the device table that take wrote: a record's
 * stream is the one whose slice [first_record, first_record + n_records) holds it (empty slices occur between non-empty ones).
 * d_sec_nsec [n_records][2] (or NULL) = stamp / 10^9 truncated to 32 bits, stamp % 10^9: the reference's time_sec / time_nsec fields. */
int cc_firing_stamps_of_points(cc_firing_stamps* h, int64_t n_records, const cc_take_point* d_records, const cc_take_stream* d_table,
                               uint64_t* d_stamps, uint32_t* d_sec_nsec);
/* _of_columns: d_column_stamps is ordered by stream, then column: the entry of global column c of stream s is at
 * sum over t < s of (col_to - col_from) + (c - col_from); the kernels derive those offsets from d_table. Each entry is the minimum non-zero
 * stamp of the column's records, 0 where the column has no record or only zero stamps. d_stream_stamps [S] is the same rule over the
 * stream's whole slice: the header stamp of the reference's one columnToPointCloud(a, b) message per publish. Either output may be NULL.
 * h_table: the host table of the same take, read for the number of columns only; NULL = d_table is copied back first, which synchronises. */
int cc_firing_stamps_of_columns(cc_firing_stamps* h, int64_t n_records, const cc_take_point* d_records, const cc_take_stream* d_table,
                                const cc_take_stream* h_table, uint64_t* d_column_stamps, uint64_t* d_stream_stamps);
/* _of_clusters: d_out[k] for descriptor k of a cc_engine_take_clusters; its stream comes from the descriptor, its members are
 * d_records[first_record .. first_record + n_points). Stamps need the records: after a take with CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY there is
 * nothing to resolve, and d_records == NULL with n_records > 0 is refused. d_point_stamps [n_records] (or NULL) receives every member's
 * stamp. A descriptor without members gets all zeros. */
int cc_firing_stamps_of_clusters(cc_firing_stamps* h, int use_last_point, int64_t n_clusters, const cc_take_cluster* d_clusters,
                                 int64_t n_records, const cc_take_point* d_records, cc_cluster_stamp* d_out, uint64_t* d_point_stamps);

#ifdef __cplusplus
}
#endif
#endif
