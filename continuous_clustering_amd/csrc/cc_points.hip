// cc_points.hip — generic PointCloud2 firings -> engine firings on gfx950 (include/cc_points.h).
//
// One kernel, k_points_decode: a byte-granular strided gather (fields sit at arbitrary byte offsets of points at arbitrary strides; the
// reference's own 37-byte point puts floats at odd addresses) plus, for organised clouds, a transpose from the message's row-major order
// into the engine's firing-major order. A 256-thread workgroup produces `tile` consecutive firings of one stream:
//   1. the bytes that hold fields are staged into LDS in contiguous SEGMENTS. Path 2 (columns == 1, the reference's message): one segment
//      per message, [first field byte of row 0, last field byte of row H-1], `tile` messages per workgroup. Path 1 (row-major organised
//      cloud): one segment per row, the field bytes of the tile's columns in that row, H segments. A segment starting at global address g
//      is read as the 16-byte words of [g & ~15, ..): every load is a naturally aligned 16-byte load whatever the alignment of the message,
//      and the byte at global address x lands at LDS offset x - (g & ~15) of the segment's image, so the image keeps the segment's phase
//      (g & 15). A word that is not entirely inside the caller's array [d_messages, d_messages + S * n_messages * message_stride) — only
//      the first and the last word of the whole array can be — is read byte by byte, and only the segment's own bytes. No misaligned
//      pointer is ever formed and nothing outside the caller's array is read.
//   2. lane (j, g) produces engine rows 4g .. 4g+3 of firing j: each f32 field is assembled from the two aligned LDS dwords that hold
//      it and a byte shift, the intensity field by its mode; 48 contiguous bytes of xyz leave as three 16-byte stores, 4 bytes of
//      intensity as one dword store, so a firing (12 H + H bytes) is written by H / 4 consecutive lanes.
//   3. nf * 6 lanes copy the message pose (16 B each) to the firings.
// Path 0 (column-major and everything whose segments would not fit in LDS) skips 1. and gathers every field byte from global memory
// with byte loads: correct for any strides, not fast. Results never depend on the path or the tile.
// The LDS budget per workgroup is 38 KB, so at least 4 workgroups (16 waves) share a CU's 160 KB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/cc_hip.h"
#include "../../include/cc_points.h"

namespace
{

thread_local std::string g_points_error;

int fail(int code, const std::string& what)
{
    g_points_error = what;
    return code;
}

#define POINTS_HIP_CHECK(expr)                                                                         \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(CC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));             \
    } while (0)

constexpr int BLOCK = 256;
constexpr int MAX_TILE = 256;        // firings per workgroup at most: 4 rows per lane, 4-row firings
constexpr int MAX_COLUMN_TILE = 64;  // columns per workgroup on the row-major path at most
constexpr int LDS_BUDGET = 38912;    // bytes of staging per workgroup: 4 workgroups in a CU's 160 KB
constexpr uint32_t QNAN_BITS = 0x7FC00000u; // __builtin_nanf("")

enum
{
    PATH_GATHER = 0,
    PATH_ROWS = 1,
    PATH_MESSAGES = 2
};

enum
{
    CNT_SKIPPED = 0,
    CNT_NO_RETURN = 1,
    NUM_COUNTERS = 2
};

struct Plan
{
    int path = PATH_GATHER;
    int tile = 1;     // firings per workgroup
    int lo = 0;       // first field byte of a point
    int span = 0;     // bytes from the first to behind the last field byte of a point
    int lds_seg = 0;  // bytes of LDS per segment image
    int lds_bytes = 0;
};

struct DecodeArgs
{
    const unsigned char* messages;  // [S][M][stride], any alignment
    const double* message_poses;    // [S][M][12] or null
    const unsigned char* skip;      // [S][M] or null
    uint32_t* xyz;                  // [S][M*C][H][3] f32 bit patterns
    unsigned char* intensity;       // [S][M*C][H]
    double* poses;                  // [S][M*C][12]
    unsigned long long* counters;   // [S][NUM_COUNTERS]
    long long message_stride, row_stride, column_stride;
    long long array_bytes;          // S * M * stride
    int n_messages, rows, columns;
    int off_x, off_y, off_z, off_i, mode, reverse;
    int path, tile, lo, span, lds_seg, tiles_per_message;
};

// an f32's bits from an LDS image at any byte offset: the two aligned dwords that hold it, shifted (the dword behind the last field byte
// of a segment is inside the image's slack; what it holds is shifted out)
__device__ __forceinline__ uint32_t lds_u32(const unsigned char* img, int at)
{
    const uint32_t* w = (const uint32_t*) (img + (at & ~3));
    return (uint32_t) ((((uint64_t) w[1] << 32) | w[0]) >> (8 * (at & 3)));
}

__device__ __forceinline__ uint32_t global_u32(const unsigned char* p)
{
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

// raw: the field's first byte (modes 0, 1) or its four bytes (modes 2, 3)
__device__ __forceinline__ uint32_t intensity_of(int mode, uint32_t raw)
{
    if (mode == CC_POINTS_INTENSITY_REFERENCE)
        return (raw * 255u) & 0xFFu; // static_cast<uint8_t>(*it * 255) on a uint8_t iterator (generic_points_input.hpp:46)
    if (mode == CC_POINTS_INTENSITY_U8)
        return raw & 0xFFu;
    const float v = __uint_as_float(raw);
    if (mode == CC_POINTS_INTENSITY_F32_UNIT)
    {
        // as k_kitti_firings: static_cast<uint8_t>(i * 255) goes through a 32-bit integer on x86-64 and keeps the low byte; values
        // outside the int32 range (and NaN) give 0x80000000 there, low byte 0
        const float p = __fmul_rn(v, 255.f);
        const int iv = (p > -2147483648.f && p < 2147483648.f) ? (int) p : (int) 0x80000000;
        return (uint32_t) iv & 0xFFu;
    }
    if (!(v > 0.f)) // NaN, zero and below
        return 0u;
    return v >= 255.f ? 255u : (uint32_t) (int) v;
}

__global__ __launch_bounds__(BLOCK) void k_points_decode(DecodeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_img[];
    __shared__ unsigned char s_skip[MAX_TILE];
    const int tid = threadIdx.x, s = blockIdx.y, H = a.rows, C = a.columns;
    const int n = a.n_messages * C; // firings per stream
    int f0, nf, c0 = 0;
    if (a.path == PATH_ROWS)
    {
        const int m = blockIdx.x / a.tiles_per_message;
        c0 = (blockIdx.x - m * a.tiles_per_message) * a.tile;
        f0 = m * C + c0;
        nf = min(a.tile, C - c0);
    }
    else
    {
        f0 = blockIdx.x * a.tile;
        nf = min(a.tile, n - f0);
    }
    const unsigned char* msgs = a.messages + (size_t) s * a.n_messages * (size_t) a.message_stride;
    const unsigned char* skip = a.skip ? a.skip + (size_t) s * a.n_messages : nullptr;
    unsigned long long* cnt = a.counters + (size_t) s * NUM_COUNTERS;

    if (tid < nf)
    {
        const int f = f0 + tid, m = f / C;
        const bool skipped = skip && skip[m];
        s_skip[tid] = skipped;
        if (skipped && f - m * C == 0) // once per message
            atomicAdd(cnt + CNT_SKIPPED, 1ull);
    }
    __syncthreads();

    // 1. stage the segments
    if (a.path != PATH_GATHER)
    {
        const bool by_rows = a.path == PATH_ROWS;
        const int nseg = by_rows ? (s_skip[0] ? 0 : H) : nf;
        const long long L = by_rows ? (nf - 1) * a.column_stride + a.span : (H - 1) * a.row_stride + a.span;
        const int nw = a.lds_seg >> 4;
        const uintptr_t array_begin = (uintptr_t) a.messages, array_end = array_begin + (uintptr_t) a.array_bytes;
        for (int idx = tid; idx < nseg * nw; idx += BLOCK)
        {
            const int k = idx / nw, i = idx - k * nw;
            if (!by_rows && s_skip[k])
                continue;
            const unsigned char* g = by_rows ? msgs + (size_t) (f0 / C) * (size_t) a.message_stride + (size_t) k * (size_t) a.row_stride +
                                                   (size_t) c0 * (size_t) a.column_stride + a.lo
                                             : msgs + (size_t) (f0 + k) * (size_t) a.message_stride + a.lo;
            const uintptr_t ga = (uintptr_t) g, w = (ga & ~(uintptr_t) 15) + 16u * (uintptr_t) i;
            if (w >= ga + (uintptr_t) L)
                continue;
            unsigned char* dst = s_img + k * a.lds_seg + 16 * i;
            if (w >= array_begin && w + 16 <= array_end)
                *(uint4*) dst = *(const uint4*) w;
            else
                for (int b = 0; b < 16; b++)
                    if (w + b >= ga && w + b < ga + (uintptr_t) L)
                        dst[b] = *(const unsigned char*) (w + b);
        }
    }
    __syncthreads();

    // 2. lane (j, g): engine rows 4g .. 4g+3 of firing f0 + j
    const int lanes_per_firing = H >> 2;
    const int has_i = a.off_i >= 0, wide_i = a.mode >= CC_POINTS_INTENSITY_F32_UNIT;
    unsigned no_return = 0;
    for (int it = tid; it < nf * lanes_per_firing; it += BLOCK)
    {
        const int j = it / lanes_per_firing, g = it - j * lanes_per_firing;
        const int f = f0 + j, m = f / C, c = f - m * C;
        uint32_t v[12];
#pragma unroll
        for (int i = 0; i < 12; i++)
            v[i] = QNAN_BITS;
        uint32_t packed = 0;
        if (!s_skip[j])
        {
            const unsigned char* msg = msgs + (size_t) m * (size_t) a.message_stride;
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const int e = 4 * g + k, r = a.reverse ? H - 1 - e : e;
                uint32_t x, y, z, raw = 0;
                if (a.path == PATH_GATHER)
                {
                    const unsigned char* p = msg + (size_t) r * (size_t) a.row_stride + (size_t) c * (size_t) a.column_stride;
                    x = global_u32(p + a.off_x);
                    y = global_u32(p + a.off_y);
                    z = global_u32(p + a.off_z);
                    if (has_i)
                        raw = wide_i ? global_u32(p + a.off_i) : (uint32_t) p[a.off_i];
                }
                else
                {
                    // the segment's image keeps the phase of its first byte's global address
                    const bool by_rows = a.path == PATH_ROWS;
                    const uintptr_t seg_start = by_rows ? (uintptr_t) msg + (uintptr_t) r * (uintptr_t) a.row_stride +
                                                              (uintptr_t) c0 * (uintptr_t) a.column_stride + a.lo
                                                        : (uintptr_t) msg + a.lo;
                    const int at = (by_rows ? r : j) * a.lds_seg + (int) (seg_start & 15) +
                                   (by_rows ? j * (int) a.column_stride : r * (int) a.row_stride) - a.lo;
                    x = lds_u32(s_img, at + a.off_x);
                    y = lds_u32(s_img, at + a.off_y);
                    z = lds_u32(s_img, at + a.off_z);
                    if (has_i)
                        raw = wide_i ? lds_u32(s_img, at + a.off_i) : (uint32_t) s_img[at + a.off_i];
                }
                v[3 * k + 0] = x;
                v[3 * k + 1] = y;
                v[3 * k + 2] = z;
                no_return += (x & 0x7FFFFFFFu) > 0x7F800000u;
                if (has_i)
                    packed |= intensity_of(a.mode, raw) << (8 * k);
            }
        }
        const size_t firing = (size_t) s * n + f;
        uint4* xyz = (uint4*) (a.xyz + firing * (size_t) (H * 3) + 12 * g);
        xyz[0] = make_uint4(v[0], v[1], v[2], v[3]);
        xyz[1] = make_uint4(v[4], v[5], v[6], v[7]);
        xyz[2] = make_uint4(v[8], v[9], v[10], v[11]);
        *(uint32_t*) (a.intensity + firing * (size_t) H + 4 * g) = packed;
    }

    // 3. the message's pose replicated to its firings, 16 B per lane
    if (a.message_poses)
        for (int it = tid; it < nf * 6; it += BLOCK)
        {
            const int j = it / 6, q = it - j * 6;
            const int f = f0 + j, m = f / C;
            const double2* src = (const double2*) (a.message_poses + ((size_t) s * a.n_messages + m) * 12);
            double2* dst = (double2*) (a.poses + ((size_t) s * n + f) * 12);
            dst[q] = src[q];
        }

    for (int o = 32; o > 0; o >>= 1)
        no_return += __shfl_down(no_return, o);
    if ((tid & 63) == 0 && no_return)
        atomicAdd(cnt + CNT_NO_RETURN, (unsigned long long) no_return);
}

int lds_segment_bytes(long long seg_len)
{
    // the image starts at the segment's phase (<= 15) and is read one dword past the last field byte; an odd number of 16-byte slots
    // keeps the rows of path 1 from all starting on one bank
    long long b = ((seg_len + 15 + 15) / 16) * 16 + 16;
    if ((b / 16) % 2 == 0)
        b += 16;
    return b > LDS_BUDGET ? LDS_BUDGET + 1 : (int) b;
}

// l is valid
Plan make_plan(const cc_points_layout& l)
{
    Plan p;
    const bool has_i = l.off_intensity >= 0;
    const long long size_i = l.intensity_mode >= CC_POINTS_INTENSITY_F32_UNIT ? 4 : 1;
    const long long lo = std::min<long long>({l.off_x, l.off_y, l.off_z, has_i ? l.off_intensity : INT32_MAX});
    const long long span = std::max<long long>({l.off_x + 4ll, l.off_y + 4ll, l.off_z + 4ll, has_i ? l.off_intensity + size_i : 0}) - lo;
    const int H = l.rows;
    p.path = PATH_GATHER;
    p.tile = 1024 / H;
    if (span >= LDS_BUDGET)
        return p;
    p.lo = (int) lo;
    p.span = (int) span;
    if (l.columns == 1)
    {
        const long long L = (H - 1) * l.row_stride + span; // (H - 1) * row_stride <= message_bytes: no overflow
        const int seg = L < LDS_BUDGET ? lds_segment_bytes(L) : LDS_BUDGET + 1;
        const int tile = std::min(1024 / H, LDS_BUDGET / seg);
        if (tile >= 1)
        {
            p.path = PATH_MESSAGES;
            p.tile = tile;
            p.lds_seg = seg;
            p.lds_bytes = tile * seg;
        }
    }
    else if (l.column_stride < l.row_stride)
    {
        int tile = MAX_COLUMN_TILE;
        while (tile / 2 >= l.columns)
            tile /= 2;
        for (; tile >= 1; tile /= 2)
        {
            if (tile > 1 && l.column_stride >= LDS_BUDGET)
                continue;
            const long long L = (tile - 1) * l.column_stride + span;
            if (L < LDS_BUDGET && (long long) H * lds_segment_bytes(L) <= LDS_BUDGET)
            {
                p.path = PATH_ROWS;
                p.tile = tile;
                p.lds_seg = lds_segment_bytes(L);
                p.lds_bytes = H * p.lds_seg;
                break;
            }
        }
    }
    return p;
}

int layout_check(const cc_points_layout* l)
{
    if (!l)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: null layout");
    if (l->rows < 4 || l->rows > 128 || l->rows % 4 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: rows must be a multiple of 4 in 4..128, not " + std::to_string(l->rows));
    if (l->columns < 1)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: columns must be >= 1, not " + std::to_string(l->columns));
    if (l->row_stride <= 0 || l->column_stride <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: row_stride and column_stride must be positive");
    if (l->intensity_mode < CC_POINTS_INTENSITY_REFERENCE || l->intensity_mode > CC_POINTS_INTENSITY_F32_255)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: unknown intensity mode " + std::to_string(l->intensity_mode));
    if (l->off_intensity < -1)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: off_intensity must be a byte offset or -1");
    if (l->message_bytes <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points: message_bytes must be positive");
    const __int128 last_point = (__int128) (l->rows - 1) * l->row_stride + (__int128) (l->columns - 1) * l->column_stride;
    const struct
    {
        const char* name;
        int off, size;
    } fields[4] = {{"x", l->off_x, 4},
                   {"y", l->off_y, 4},
                   {"z", l->off_z, 4},
                   {"intensity", l->off_intensity, l->intensity_mode >= CC_POINTS_INTENSITY_F32_UNIT ? 4 : 1}};
    for (int i = 0; i < 4; i++)
    {
        if (i == 3 && fields[i].off == -1)
            continue;
        if (fields[i].off < 0 || last_point + fields[i].off + fields[i].size > (__int128) l->message_bytes)
            return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_points: field ") + fields[i].name + " (offset " +
                                                     std::to_string(fields[i].off) + ", " + std::to_string(fields[i].size) +
                                                     " bytes) does not lie inside [0, message_bytes) for every row and column");
    }
    return CC_OK;
}

} // namespace

struct cc_points
{
    int device = 0;
    int num_streams = 0;
    int max_messages = 0;
    cc_points_layout layout{};
    Plan plan;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    unsigned long long* d_counters = nullptr; // [S][NUM_COUNTERS]
};

extern "C" {

const char* cc_points_last_error(void)
{
    return g_points_error.c_str();
}

int cc_points_layout_check(const cc_points_layout* layout)
{
    return layout_check(layout);
}

int cc_points_path(const cc_points_layout* layout)
{
    return layout_check(layout) == CC_OK ? make_plan(*layout).path : -1;
}

int cc_points_column_tile(const cc_points_layout* layout)
{
    return layout_check(layout) == CC_OK ? make_plan(*layout).tile : -1;
}

int cc_points_create(cc_points** out, int device, int num_streams, const cc_points_layout* layout, int max_messages, void* hip_stream)
{
    if (!out)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_create: null output handle");
    *out = nullptr;
    if (num_streams <= 0 || max_messages <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_create: num_streams and max_messages must be positive");
    if (num_streams > 65535)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_create: at most 65535 streams (the grid's second dimension)");
    const int rc = layout_check(layout);
    if (rc != CC_OK)
        return rc;
    if ((long long) max_messages * layout->columns > INT32_MAX)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_create: max_messages * columns firings per call do not fit in 31 bits");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(CC_ERR_NO_DEVICE, "cc_points_create: no gfx950 device (there is no CPU variant of this path)");
    POINTS_HIP_CHECK(hipSetDevice(device));
    cc_points* o = new cc_points;
    o->device = device;
    o->num_streams = num_streams;
    o->max_messages = max_messages;
    o->layout = *layout;
    o->plan = make_plan(*layout);
    if (hip_stream)
        o->stream = (hipStream_t) hip_stream;
    else
    {
        POINTS_HIP_CHECK(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
        o->own_stream = true;
    }
    POINTS_HIP_CHECK(hipMalloc(&o->d_counters, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    POINTS_HIP_CHECK(hipMemset(o->d_counters, 0, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    *out = o;
    return CC_OK;
}

void cc_points_destroy(cc_points* o)
{
    if (!o)
        return;
    (void) hipSetDevice(o->device);
    (void) hipStreamSynchronize(o->stream);
    if (o->d_counters)
        (void) hipFree(o->d_counters);
    if (o->own_stream)
        (void) hipStreamDestroy(o->stream);
    delete o;
}

void* cc_points_hip_stream(cc_points* o)
{
    return o ? (void*) o->stream : nullptr;
}

int cc_points_sync(cc_points* o)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    POINTS_HIP_CHECK(hipSetDevice(o->device));
    POINTS_HIP_CHECK(hipStreamSynchronize(o->stream));
    return CC_OK;
}

int cc_points_decode(cc_points* o, int n_messages, const uint8_t* d_messages, int64_t message_stride, const double* d_message_poses,
                     const uint8_t* d_skip, float* d_xyz, uint8_t* d_intensity, double* d_poses)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    const cc_points_layout& l = o->layout;
    if (n_messages < 1 || n_messages > o->max_messages)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_decode: n_messages " + std::to_string(n_messages) + " not in 1..max_messages (" +
                                                 std::to_string(o->max_messages) + ")");
    if (message_stride < l.message_bytes)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_decode: message_stride " + std::to_string(message_stride) +
                                                 " is below message_bytes " + std::to_string(l.message_bytes));
    if ((__int128) message_stride * n_messages * o->num_streams > (__int128) INT64_MAX)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_decode: message_stride * n_messages * streams does not fit in 63 bits");
    if (!d_messages || !d_xyz || !d_intensity || (d_message_poses && !d_poses))
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_points_decode: d_messages, d_xyz, d_intensity (and d_poses with d_message_poses) are required");
    auto misaligned = [](const void* p, uintptr_t a) { return p && ((uintptr_t) p % a) != 0; };
    if (misaligned(d_xyz, 16) || misaligned(d_intensity, 4) || misaligned(d_poses, 16) || misaligned(d_message_poses, 16))
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_points_decode: misaligned buffer (xyz / poses / message poses 16 B, intensity 4 B; messages may sit anywhere)");
    const Plan& p = o->plan;
    const long long firings = (long long) n_messages * l.columns;
    const int tiles_per_message = (l.columns + p.tile - 1) / p.tile;
    const long long groups = p.path == PATH_ROWS ? (long long) n_messages * tiles_per_message : (firings + p.tile - 1) / p.tile;
    if (groups > INT32_MAX)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_decode: too many workgroups for one launch; decode fewer messages per call");
    POINTS_HIP_CHECK(hipSetDevice(o->device));
    DecodeArgs a;
    a.messages = d_messages;
    a.message_poses = d_message_poses;
    a.skip = d_skip;
    a.xyz = (uint32_t*) d_xyz;
    a.intensity = d_intensity;
    a.poses = d_poses;
    a.counters = o->d_counters;
    a.message_stride = message_stride;
    a.row_stride = l.row_stride;
    a.column_stride = l.column_stride;
    a.array_bytes = (long long) message_stride * n_messages * o->num_streams;
    a.n_messages = n_messages;
    a.rows = l.rows;
    a.columns = l.columns;
    a.off_x = l.off_x;
    a.off_y = l.off_y;
    a.off_z = l.off_z;
    a.off_i = l.off_intensity;
    a.mode = l.intensity_mode;
    a.reverse = l.reverse_rows != 0;
    a.path = p.path;
    a.tile = p.tile;
    a.lo = p.lo;
    a.span = p.span;
    a.lds_seg = p.lds_seg;
    a.tiles_per_message = tiles_per_message;
    hipLaunchKernelGGL(k_points_decode, dim3((unsigned) groups, o->num_streams), dim3(BLOCK), (size_t) p.lds_bytes, o->stream, a);
    POINTS_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_points_counters(cc_points* o, int stream, uint64_t* skipped_messages, uint64_t* no_return_points)
{
    if (!o || stream < 0 || stream >= o->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_counters: no such stream");
    POINTS_HIP_CHECK(hipSetDevice(o->device));
    POINTS_HIP_CHECK(hipStreamSynchronize(o->stream));
    unsigned long long v[NUM_COUNTERS];
    POINTS_HIP_CHECK(hipMemcpy(v, o->d_counters + (size_t) stream * NUM_COUNTERS, sizeof(v), hipMemcpyDeviceToHost));
    if (skipped_messages)
        *skipped_messages = v[CNT_SKIPPED];
    if (no_return_points)
        *no_return_points = v[CNT_NO_RETURN];
    return CC_OK;
}

int cc_points_check_engine(cc_points* o, struct cc_engine* e)
{
    if (!o || !e)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_check_engine: null handle");
    cc_stream_state st;
    int rc = cc_engine_stream_state(e, o->num_streams - 1, &st);
    if (rc == CC_ERR_INVALID_ARGUMENT || (rc == CC_OK && cc_engine_stream_state(e, o->num_streams, &st) == CC_OK))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_check_engine: the engine does not have " + std::to_string(o->num_streams) + " streams");
    if (rc != CC_OK)
        return fail(rc, std::string("cc_points_check_engine: ") + cc_engine_last_error(e));
    if (st.num_rows != o->layout.rows)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_points_check_engine: the decoder has " + std::to_string(o->layout.rows) +
                                                 " rows, the engine " + std::to_string(st.num_rows));
    return CC_OK;
}

} // extern "C"
