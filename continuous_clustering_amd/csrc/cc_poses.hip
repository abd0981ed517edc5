// cc_poses.hip — per-firing odometry poses interpolated on gfx950 from pose tracks (include/cc_poses.h).
//
// Two kernels over one shared function, ccp::interpolate (cc_pose_math.h), which the host twin calls too: one thread per query, grid
// (ceil(n / 256), streams). A thread finds its interval by binary search over its stream's stamps (in a sweep the 64 lanes of a wave
// walk the same path: 2200 firings fall into two or three intervals), runs the slerp and writes its pose as six 16-byte stores. The
// kernels are bound by what they write, 96 B per firing; nothing is staged in LDS and there are no atomics.
// Host side: the tracks live in device memory, [S][max_samples] stamps and [S][max_samples][12] poses; the sample counts are known on the
// host and travel with each call. What a call copies from the caller's host arrays goes through pinned staging owned by the handle: one
// buffer for cc_pose_tracks_set, a ring of slots for the per-call stream parameters, each guarded by an event so that a slot is not
// rewritten before its upload has run.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cc_hip.h"
#include "../../include/cc_poses.h"
#include "cc_pose_math.h"

namespace
{

thread_local std::string g_poses_error;

int fail(int code, const std::string& what)
{
    g_poses_error = what;
    return code;
}

#define POSES_HIP_CHECK(expr)                                                                          \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(CC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));             \
    } while (0)

constexpr int BLOCK = 256;
constexpr int PARAM_SLOTS = 4;

struct StreamParams // per stream and call
{
    uint64_t start, end; // sweep only
    int32_t count;       // samples of the track
    int32_t hold;        // sweep only: -1 or the sample to repeat
};

__device__ __forceinline__ void store_pose(double* dst, const double* p)
{
    double2* d = (double2*) dst;
#pragma unroll
    for (int i = 0; i < 6; i++)
        d[i] = make_double2(p[2 * i], p[2 * i + 1]);
}

__global__ __launch_bounds__(BLOCK) void k_pose_sweep(const StreamParams* params, const uint64_t* track_stamps, const double* track_poses,
                                                       int max_samples, int n, double* poses, uint64_t* stamps)
{
    const int c = blockIdx.x * BLOCK + threadIdx.x, s = blockIdx.y;
    if (c >= n)
        return;
    const StreamParams p = params[s];
    const uint64_t* ts = track_stamps + (size_t) s * max_samples;
    const double* tp = track_poses + (size_t) s * max_samples * 12;
    const uint64_t stamp = ccp::sweep_stamp(p.start, p.end, c, n);
    double out[12];
    if (p.hold >= 0)
    {
#pragma unroll
        for (int i = 0; i < 12; i++)
            out[i] = tp[(size_t) p.hold * 12 + i];
    }
    else
        ccp::interpolate(p.count, ts, tp, stamp, out);
    const size_t at = (size_t) s * n + c;
    store_pose(poses + at * 12, out);
    if (stamps)
        stamps[at] = stamp;
}

__global__ __launch_bounds__(BLOCK) void k_pose_lookup(const StreamParams* params, const uint64_t* track_stamps, const double* track_poses,
                                                        int max_samples, int n, const uint64_t* query_stamps, int repeat, double* poses)
{
    const int q = blockIdx.x * BLOCK + threadIdx.x, s = blockIdx.y;
    if (q >= n)
        return;
    const uint64_t* ts = track_stamps + (size_t) s * max_samples;
    const double* tp = track_poses + (size_t) s * max_samples * 12;
    double out[12];
    ccp::interpolate(params[s].count, ts, tp, query_stamps[(size_t) s * n + q], out);
    double* dst = poses + ((size_t) s * n + q) * (size_t) repeat * 12;
    for (int r = 0; r < repeat; r++)
        store_pose(dst + (size_t) r * 12, out);
}

} // namespace

struct cc_pose_tracks
{
    int device = 0;
    int num_streams = 0;
    int max_samples = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<int32_t> count;       // samples per stream, 0 = never set
    uint64_t* d_stamps = nullptr;     // [S][max_samples]
    double* d_poses = nullptr;        // [S][max_samples][12]
    unsigned char* h_set = nullptr;   // pinned: max_samples stamps, then max_samples poses
    hipEvent_t set_done = nullptr;    // the upload out of h_set has run
    bool set_pending = false;
    StreamParams* h_params = nullptr; // pinned [PARAM_SLOTS][S]
    StreamParams* d_params = nullptr; // [PARAM_SLOTS][S]
    hipEvent_t params_done[PARAM_SLOTS] = {};
    bool params_pending[PARAM_SLOTS] = {};
    int next_slot = 0;
};

namespace
{

void release(cc_pose_tracks* h)
{
    (void) hipSetDevice(h->device);
    if (h->stream)
        (void) hipStreamSynchronize(h->stream);
    if (h->d_stamps)
        (void) hipFree(h->d_stamps);
    if (h->d_poses)
        (void) hipFree(h->d_poses);
    if (h->d_params)
        (void) hipFree(h->d_params);
    if (h->h_set)
        (void) hipHostFree(h->h_set);
    if (h->h_params)
        (void) hipHostFree(h->h_params);
    if (h->set_done)
        (void) hipEventDestroy(h->set_done);
    for (hipEvent_t e : h->params_done)
        if (e)
            (void) hipEventDestroy(e);
    if (h->own_stream && h->stream)
        (void) hipStreamDestroy(h->stream);
    delete h;
}

int create(cc_pose_tracks* h, void* hip_stream)
{
    POSES_HIP_CHECK(hipSetDevice(h->device));
    if (hip_stream)
        h->stream = (hipStream_t) hip_stream;
    else
    {
        POSES_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    const size_t S = (size_t) h->num_streams, M = (size_t) h->max_samples;
    POSES_HIP_CHECK(hipMalloc(&h->d_stamps, S * M * sizeof(uint64_t)));
    POSES_HIP_CHECK(hipMalloc(&h->d_poses, S * M * 12 * sizeof(double)));
    POSES_HIP_CHECK(hipMalloc(&h->d_params, PARAM_SLOTS * S * sizeof(StreamParams)));
    POSES_HIP_CHECK(hipHostMalloc(&h->h_set, M * (sizeof(uint64_t) + 12 * sizeof(double)), hipHostMallocDefault));
    POSES_HIP_CHECK(hipHostMalloc(&h->h_params, PARAM_SLOTS * S * sizeof(StreamParams), hipHostMallocDefault));
    POSES_HIP_CHECK(hipEventCreateWithFlags(&h->set_done, hipEventDisableTiming));
    for (hipEvent_t& e : h->params_done)
        POSES_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return CC_OK;
}

// the next parameter slot, free to be written: *host is its pinned image, *dev where upload_params puts it
int take_params_slot(cc_pose_tracks* h, StreamParams** host, StreamParams** dev, int* slot)
{
    const int k = h->next_slot;
    if (h->params_pending[k])
    {
        POSES_HIP_CHECK(hipEventSynchronize(h->params_done[k]));
        h->params_pending[k] = false;
    }
    *host = h->h_params + (size_t) k * h->num_streams;
    *dev = h->d_params + (size_t) k * h->num_streams;
    *slot = k;
    return CC_OK;
}

int upload_params(cc_pose_tracks* h, int slot)
{
    const size_t bytes = (size_t) h->num_streams * sizeof(StreamParams);
    POSES_HIP_CHECK(hipMemcpyAsync(h->d_params + (size_t) slot * h->num_streams, h->h_params + (size_t) slot * h->num_streams, bytes,
                                   hipMemcpyHostToDevice, h->stream));
    POSES_HIP_CHECK(hipEventRecord(h->params_done[slot], h->stream));
    h->params_pending[slot] = true;
    h->next_slot = (slot + 1) % PARAM_SLOTS;
    return CC_OK;
}

int unset_stream(const cc_pose_tracks* h)
{
    for (int s = 0; s < h->num_streams; s++)
        if (h->count[s] == 0)
            return s;
    return -1;
}

} // namespace

extern "C" {

const char* cc_poses_last_error(void)
{
    return g_poses_error.c_str();
}

int cc_poses_host_lookup(int64_t n_samples, const uint64_t* stamps, const double* poses, int64_t n_queries, const uint64_t* query_stamps,
                         double* out_poses)
{
    if (n_samples <= 0 || !stamps || !poses || n_queries < 0 || (n_queries > 0 && (!query_stamps || !out_poses)))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_poses_host_lookup: bad argument");
    for (int64_t q = 0; q < n_queries; q++)
        ccp::interpolate(n_samples, stamps, poses, query_stamps[q], out_poses + (size_t) q * 12);
    return CC_OK;
}

int cc_poses_host_sweep(int64_t n_samples, const uint64_t* stamps, const double* poses, int32_t n, uint64_t start, uint64_t end,
                        uint64_t* out_stamps, double* out_poses)
{
    if (n_samples <= 0 || !stamps || !poses || end < start)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_poses_host_sweep: bad argument");
    if (n < 2)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_poses_host_sweep: a sweep has at least 2 firings, not " + std::to_string(n));
    for (int c = 0; c < n; c++)
    {
        const uint64_t stamp = ccp::sweep_stamp(start, end, c, n);
        if (out_stamps)
            out_stamps[c] = stamp;
        if (out_poses)
            ccp::interpolate(n_samples, stamps, poses, stamp, out_poses + (size_t) c * 12);
    }
    return CC_OK;
}

int cc_pose_tracks_create(cc_pose_tracks** out, int device, int num_streams, int max_samples, void* hip_stream)
{
    if (!out)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_create: null output handle");
    *out = nullptr;
    if (num_streams <= 0 || max_samples <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_create: num_streams and max_samples must be positive");
    if (num_streams > 65535)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_create: at most 65535 streams (the grid's second dimension)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(CC_ERR_NO_DEVICE, "cc_pose_tracks_create: no gfx950 device (there is no CPU variant of this path)");
    cc_pose_tracks* h = new cc_pose_tracks;
    h->device = device;
    h->num_streams = num_streams;
    h->max_samples = max_samples;
    h->count.assign((size_t) num_streams, 0);
    const int rc = create(h, hip_stream);
    if (rc != CC_OK)
    {
        release(h);
        return rc;
    }
    *out = h;
    return CC_OK;
}

void cc_pose_tracks_destroy(cc_pose_tracks* h)
{
    if (h)
        release(h);
}

void* cc_pose_tracks_hip_stream(cc_pose_tracks* h)
{
    return h ? (void*) h->stream : nullptr;
}

int cc_pose_tracks_sync(cc_pose_tracks* h)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sync: null handle");
    POSES_HIP_CHECK(hipSetDevice(h->device));
    POSES_HIP_CHECK(hipStreamSynchronize(h->stream));
    return CC_OK;
}

int cc_pose_tracks_set(cc_pose_tracks* h, int stream, int n, const uint64_t* stamps, const double* poses)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_set: null handle");
    if (stream < 0 || stream >= h->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_set: no such stream " + std::to_string(stream));
    if (n < 1 || n > h->max_samples)
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_pose_tracks_set: " + std::to_string(n) + " samples not in 1..max_samples (" + std::to_string(h->max_samples) + ")");
    if (!stamps || !poses)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_set: stamps and poses are required");
    for (int i = 1; i < n; i++)
        if (stamps[i] < stamps[i - 1])
            return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_set: stamps decrease at sample " + std::to_string(i));
    POSES_HIP_CHECK(hipSetDevice(h->device));
    if (h->set_pending)
    {
        POSES_HIP_CHECK(hipEventSynchronize(h->set_done));
        h->set_pending = false;
    }
    const size_t M = (size_t) h->max_samples;
    uint64_t* hs = (uint64_t*) h->h_set;
    double* hp = (double*) (h->h_set + M * sizeof(uint64_t));
    std::memcpy(hs, stamps, (size_t) n * sizeof(uint64_t));
    std::memcpy(hp, poses, (size_t) n * 12 * sizeof(double));
    POSES_HIP_CHECK(hipMemcpyAsync(h->d_stamps + (size_t) stream * M, hs, (size_t) n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    POSES_HIP_CHECK(hipMemcpyAsync(h->d_poses + (size_t) stream * M * 12, hp, (size_t) n * 12 * sizeof(double), hipMemcpyHostToDevice,
                                   h->stream));
    POSES_HIP_CHECK(hipEventRecord(h->set_done, h->stream));
    h->set_pending = true;
    h->count[(size_t) stream] = n;
    return CC_OK;
}

int cc_pose_tracks_sweep(cc_pose_tracks* h, int n, const uint64_t* h_start, const uint64_t* h_end, const int32_t* h_hold, double* d_poses,
                         uint64_t* d_stamps)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: null handle");
    if (n < 2)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: a sweep has at least 2 firings, not " + std::to_string(n));
    if (!h_start || !h_end || !d_poses)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: h_start, h_end and d_poses are required");
    if ((uintptr_t) d_poses % 16 != 0 || (uintptr_t) d_stamps % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: misaligned buffer (d_poses 16 B, d_stamps 8 B)");
    const int unset = unset_stream(h);
    if (unset >= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: stream " + std::to_string(unset) + " has no track (cc_pose_tracks_set)");
    for (int s = 0; s < h->num_streams; s++)
    {
        if (h_end[s] < h_start[s])
            return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: stream " + std::to_string(s) + " ends before it starts");
        if (h_hold && (h_hold[s] < -1 || h_hold[s] >= h->count[(size_t) s]))
            return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_sweep: hold " + std::to_string(h_hold[s]) + " of stream " + std::to_string(s) +
                                                     " not in -1.." + std::to_string(h->count[(size_t) s] - 1));
    }
    POSES_HIP_CHECK(hipSetDevice(h->device));
    StreamParams *hp, *dp;
    int slot;
    int rc = take_params_slot(h, &hp, &dp, &slot);
    if (rc != CC_OK)
        return rc;
    for (int s = 0; s < h->num_streams; s++)
        hp[s] = StreamParams{h_start[s], h_end[s], h->count[(size_t) s], h_hold ? h_hold[s] : -1};
    rc = upload_params(h, slot);
    if (rc != CC_OK)
        return rc;
    hipLaunchKernelGGL(k_pose_sweep, dim3((unsigned) ((n + BLOCK - 1) / BLOCK), (unsigned) h->num_streams), dim3(BLOCK), 0, h->stream, dp,
                       h->d_stamps, h->d_poses, h->max_samples, n, d_poses, d_stamps);
    POSES_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_pose_tracks_lookup(cc_pose_tracks* h, int n, const uint64_t* d_query_stamps, int repeat, double* d_poses)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_lookup: null handle");
    if (n < 1 || repeat < 1 || (long long) n * repeat > INT32_MAX)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_lookup: n and repeat must be positive and n * repeat fit in 31 bits");
    if (!d_query_stamps || !d_poses)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_lookup: d_query_stamps and d_poses are required");
    if ((uintptr_t) d_poses % 16 != 0 || (uintptr_t) d_query_stamps % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_lookup: misaligned buffer (d_poses 16 B, d_query_stamps 8 B)");
    const int unset = unset_stream(h);
    if (unset >= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_pose_tracks_lookup: stream " + std::to_string(unset) + " has no track (cc_pose_tracks_set)");
    POSES_HIP_CHECK(hipSetDevice(h->device));
    StreamParams *hp, *dp;
    int slot;
    int rc = take_params_slot(h, &hp, &dp, &slot);
    if (rc != CC_OK)
        return rc;
    for (int s = 0; s < h->num_streams; s++)
        hp[s] = StreamParams{0, 0, h->count[(size_t) s], -1};
    rc = upload_params(h, slot);
    if (rc != CC_OK)
        return rc;
    hipLaunchKernelGGL(k_pose_lookup, dim3((unsigned) ((n + BLOCK - 1) / BLOCK), (unsigned) h->num_streams), dim3(BLOCK), 0, h->stream, dp,
                       h->d_stamps, h->d_poses, h->max_samples, n, d_query_stamps, repeat, d_poses);
    POSES_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

} // extern "C"
