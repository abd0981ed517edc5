// cc_velodyne.hip — Velodyne VLS-128 UDP payloads -> engine firings on gfx950 (include/cc_velodyne.h).
//
// One kernel, k_velodyne_decode: a 384-thread workgroup decodes 4 consecutive packets of one stream, 96 lanes per packet. A packet is
// only 384 points and 6.6 KB of traffic, and a grid of one 2-wave workgroup per packet (160 000 of them for 256 streams x one rotation)
// would be bounded by workgroup dispatch, not by HBM; 4 packets per workgroup keep the dispatcher at a quarter of that and a CU at its
// 32 waves with 5 workgroups. Pure streaming:
//   1. the packets are staged into LDS (records sit at a 3-byte stride inside 100-byte blocks, so nothing in a packet is naturally
//      aligned past its u16 fields): 16-byte loads when base and stride are multiples of 16, dword loads when multiples of 4, u16 loads
//      otherwise (a bare 1206-byte payload at a 1206-byte stride);
//   2. one lane per packet reads the 12 block headers and the return-mode byte and decides how many firing slots are valid;
//   3. lane (f, g) of a packet produces output rows 4g .. 4g+3 of firing slot f through the row -> laser map of the stream's
//      calibration: 48 contiguous bytes of xyz as three 16-byte stores, 4 bytes of intensity; 18 lanes copy the packet pose (16 B each)
//      to the 3 firings. The rotation tables (2 x 36000 floats, 288 KB) and the calibrations (128 x 16 B + 128 B each) stay in L2.
//      All trigonometry is table look-ups: no device transcendentals.
// HBM bytes per packet: read 1206 (1216 on the 16-byte path) + 96 (pose) + 1 (skip); written 3*128*12 + 3*128 + 3*96 + 3*4 = 5292.
// 6595 B per packet, 17.2 B per point.
//
// Device code is built with -ffp-contract=off and spells the driver's f32 arithmetic with __fmul_rn / __fadd_rn anyway.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cc_hip.h"
#include "../../include/cc_velodyne.h"

namespace
{

thread_local std::string g_velodyne_error;

int fail(int code, const std::string& what)
{
    g_velodyne_error = what;
    return code;
}

#define VELODYNE_HIP_CHECK(expr)                                                                       \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(CC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));             \
    } while (0)

constexpr int ROWS = 128;
constexpr int SLOTS = 3;         // firing slots (sequences of 4 blocks) per packet
constexpr int BLOCKS = 12;       // data blocks per packet
constexpr int BLOCK_BYTES = 100; // u16 header, u16 rotation, 32 x (u16 distance, u8 intensity)
constexpr int PACKET_BYTES = 1206;
constexpr int RETURN_MODE_OFFSET = 1204;
constexpr int RETURN_MODE_DUAL = 57;
constexpr int ROTATION_MAX = 36000;
constexpr float DISTANCE_RESOLUTION = 0.004f;
constexpr float FRAC_UNIT = 2.665f / 53.3f; // channel duration / sequence duration, f32 as in the driver
constexpr int LDS_SLOT = 1216;              // bytes of LDS per staged packet (76 x 16)
constexpr int PACKETS_PER_WG = 4;
constexpr int LANES_PER_PACKET = SLOTS * ROWS / 4; // 96: one lane per 4 output rows
constexpr int BLOCK = PACKETS_PER_WG * LANES_PER_PACKET;

struct StreamCal
{
    const float4* trig;                 // [128] by laser: cos_rot, sin_rot, cos_vert, sin_vert
    const unsigned char* laser_of_row;  // [128]: the laser whose point lands in output row r (127 - laser_ring[laser] == r)
};

enum
{
    CNT_BAD_HEADER = 0,
    CNT_DUAL = 1,
    CNT_SKIPPED = 2,
    NUM_COUNTERS = 3
};

struct DecodeArgs
{
    const unsigned char* packets;  // [S][P][stride]
    const double* packet_poses;    // [S][P][12] or null
    const unsigned char* skip;     // [S][P] or null
    float* xyz;                    // [S][3P][128][3]
    unsigned char* intensity;      // [S][3P][128]
    double* poses;                 // [S][3P][12]
    int* block_azimuth;            // [S][3P] or null
    const StreamCal* cals;         // [S]
    const float* cos_tab;          // [36000]
    const float* sin_tab;          // [36000]
    unsigned long long* counters;  // [S][NUM_COUNTERS]
    long long stride;
    int n_packets;
    int load_bytes; // 16, 4 or 2
};

__device__ __forceinline__ int lds_u16(const unsigned char* p)
{
    return *(const unsigned short*) p;
}

// round(): half away from zero, exact (x - trunc(x) is exact in f32)
__device__ __forceinline__ float round_half_away(float x)
{
    const float t = truncf(x);
    return fabsf(__fsub_rn(x, t)) >= 0.5f ? __fadd_rn(t, copysignf(1.f, x)) : t;
}

__global__ __launch_bounds__(BLOCK) void k_velodyne_decode(DecodeArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_pkt[PACKETS_PER_WG * LDS_SLOT];
    __shared__ int s_nvalid[PACKETS_PER_WG]; // valid firing slots of each packet, 0..3
    const int tid = threadIdx.x, q = tid / LANES_PER_PACKET, sub = tid - q * LANES_PER_PACKET;
    const int s = blockIdx.y, p = blockIdx.x * PACKETS_PER_WG + q;
    const bool in_range = p < a.n_packets;
    const size_t pk = (size_t) s * a.n_packets + (in_range ? p : 0);
    const bool skipped = in_range && a.skip && a.skip[pk];
    unsigned char* pkt = s_pkt + q * LDS_SLOT;

    // 1. stage the packet (every path reads at most `stride` bytes from the packet's base: 1216 <= stride on the 16-byte path, 1208 on
    //    the dword path, 1206 otherwise)
    if (in_range && !skipped)
    {
        const unsigned char* src = a.packets + pk * (size_t) a.stride;
        if (a.load_bytes == 16)
            for (int i = sub; i < LDS_SLOT / 16; i += LANES_PER_PACKET)
                ((uint4*) pkt)[i] = ((const uint4*) src)[i];
        else if (a.load_bytes == 4)
            for (int i = sub; i < (PACKET_BYTES + 3) / 4; i += LANES_PER_PACKET)
                ((uint32_t*) pkt)[i] = ((const uint32_t*) src)[i];
        else
            for (int i = sub; i < PACKET_BYTES / 2; i += LANES_PER_PACKET)
                ((unsigned short*) pkt)[i] = ((const unsigned short*) src)[i];
    }
    __syncthreads();

    // 2. slot validity, once per packet: the driver leaves the packet at the first block whose header is not the expected bank
    if (sub == 0 && in_range)
    {
        int nv = 0;
        bool dual = false;
        if (!skipped)
        {
            dual = pkt[RETURN_MODE_OFFSET] == RETURN_MODE_DUAL;
            bool ok = !dual;
            for (int f = 0; f < SLOTS && ok; f++)
            {
                const unsigned char* blk = pkt + 4 * f * BLOCK_BYTES;
                ok = lds_u16(blk) == 0xEEFF && lds_u16(blk + BLOCK_BYTES) == 0xDDFF && lds_u16(blk + 2 * BLOCK_BYTES) == 0xCCFF &&
                     lds_u16(blk + 3 * BLOCK_BYTES) == 0xBBFF;
                nv += ok;
            }
        }
        s_nvalid[q] = nv;
        unsigned long long* cnt = a.counters + (size_t) s * NUM_COUNTERS;
        if (skipped)
            atomicAdd(cnt + CNT_SKIPPED, 1ull);
        else if (dual)
            atomicAdd(cnt + CNT_DUAL, 1ull);
        else if (nv < SLOTS)
            atomicAdd(cnt + CNT_BAD_HEADER, (unsigned long long) (SLOTS - nv));
    }
    __syncthreads();
    if (!in_range)
        return;

    // 3. lane (f, g): rows 4g .. 4g+3 of firing slot f
    const int f = sub >> 5, g = sub & 31;
    const int nv = s_nvalid[q];
    const size_t firing0 = ((size_t) s * a.n_packets + p) * SLOTS; // first output firing of this packet
    const float qnan = __builtin_nanf("");
    float v[12];
#pragma unroll
    for (int i = 0; i < 12; i++)
        v[i] = qnan;
    uint32_t packed = 0;
    if (f < nv)
    {
        const StreamCal cal = a.cals[s];
        const uint32_t lasers = *(const uint32_t*) (cal.laser_of_row + 4 * g);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int L = (lasers >> (8 * k)) & 0xFF;
            const int b = 4 * f + (L >> 5);
            const unsigned char* blk = pkt + b * BLOCK_BYTES;
            const unsigned char* rec = blk + 4 + 3 * (L & 31);
            const int raw = rec[0] | (rec[1] << 8);
            if (raw == 0) // no return: NaN, intensity 0 (velodyne_input.hpp:69-75)
                continue;
            const int rot = lds_u16(blk + 2);
            const float diff = b < BLOCKS - 1 ? (float) ((ROTATION_MAX + lds_u16(blk + BLOCK_BYTES + 2) - rot) % ROTATION_MAX) : 0.f;
            const int order = L >> 3;
            const float frac = __fmul_rn(FRAC_UNIT, (float) (order + order / 8));
            const float a_f = __fadd_rn((float) rot, __fmul_rn(diff, frac));
            const int ai = (((int) round_half_away(a_f)) & 0xFFFF) % ROTATION_MAX; // the driver's (uint16_t) round(..) % 36000 on x86-64
            const float ct = a.cos_tab[ai], st = a.sin_tab[ai];
            const float4 c = cal.trig[L];
            const float d = __fmul_rn((float) raw, DISTANCE_RESOLUTION);
            const float cr = __fadd_rn(__fmul_rn(ct, c.x), __fmul_rn(st, c.y));
            const float sr = __fsub_rn(__fmul_rn(st, c.x), __fmul_rn(ct, c.y));
            const float xy = __fmul_rn(d, c.z);
            v[3 * k + 0] = __fmul_rn(xy, cr);
            v[3 * k + 1] = -__fmul_rn(xy, sr);
            v[3 * k + 2] = __fmul_rn(d, c.w);
            packed |= (uint32_t) rec[2] << (8 * k);
        }
    }
    float4* xyz = (float4*) (a.xyz + (firing0 + f) * (size_t) (ROWS * 3) + 12 * g);
    xyz[0] = make_float4(v[0], v[1], v[2], v[3]);
    xyz[1] = make_float4(v[4], v[5], v[6], v[7]);
    xyz[2] = make_float4(v[8], v[9], v[10], v[11]);
    *(uint32_t*) (a.intensity + (firing0 + f) * (size_t) ROWS + 4 * g) = packed;

    // the packet's pose replicated to its 3 firings, 16 B per lane; the first block's rotation word of each firing
    if (a.packet_poses && sub < SLOTS * 6)
    {
        const double2* src = (const double2*) (a.packet_poses + pk * 12);
        double2* dst = (double2*) (a.poses + firing0 * 12);
        dst[sub] = src[sub % 6];
    }
    if (a.block_azimuth && sub < SLOTS)
        a.block_azimuth[firing0 + sub] = sub < nv ? lds_u16(pkt + 4 * sub * BLOCK_BYTES + 2) : -1;
}

struct CalEntry
{
    std::vector<float> trig;    // [128][4]
    std::vector<int32_t> ring;  // [128]
    unsigned char* d = nullptr; // 128 float4, then the 128 bytes of laser_of_row
    int refs = 0;
};

constexpr size_t CAL_DEVICE_BYTES = ROWS * sizeof(float4) + ROWS;

void rotation_tables(float* cos_table, float* sin_table)
{
    for (int i = 0; i < ROTATION_MAX; i++)
    {
        const float rad = (float) ((double) (0.01f * i) * M_PI / 180.0); // angles::from_degrees(ROTATION_RESOLUTION * i), stored as float
        if (cos_table)
            cos_table[i] = cosf(rad);
        if (sin_table)
            sin_table[i] = sinf(rad);
    }
}

} // namespace

struct cc_velodyne
{
    int device = 0;
    int num_streams = 0;
    int max_packets = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float* d_tables = nullptr;                // cos then sin, 36000 floats each
    StreamCal* d_cals = nullptr;              // [S]
    unsigned long long* d_counters = nullptr; // [S][NUM_COUNTERS]
    std::vector<CalEntry> entries;
    std::vector<int> stream_entry; // index into entries, -1 = no calibration yet
};

extern "C" {

const char* cc_velodyne_last_error(void)
{
    return g_velodyne_error.c_str();
}

int64_t cc_velodyne_packet_bytes(void)
{
    return PACKET_BYTES;
}

int cc_velodyne_rows(void)
{
    return ROWS;
}

int cc_velodyne_firings_per_packet(void)
{
    return SLOTS;
}

int cc_velodyne_rotation_tables(float* cos_table, float* sin_table)
{
    rotation_tables(cos_table, sin_table);
    return CC_OK;
}

int cc_velodyne_make_calibration(int n, const double* rot_correction_rad, const double* vert_correction_rad, float* cos_rot_correction,
                                 float* sin_rot_correction, float* cos_vert_correction, float* sin_vert_correction, int32_t* laser_ring)
{
    if (n < 1 || !rot_correction_rad || !vert_correction_rad)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_make_calibration: bad argument");
    for (int i = 0; i < n; i++)
    {
        const float rot = (float) rot_correction_rad[i], vert = (float) vert_correction_rad[i]; // the driver keeps its angles as floats
        if (cos_rot_correction)
            cos_rot_correction[i] = cosf(rot);
        if (sin_rot_correction)
            sin_rot_correction[i] = sinf(rot);
        if (cos_vert_correction)
            cos_vert_correction[i] = cosf(vert);
        if (sin_vert_correction)
            sin_vert_correction[i] = sinf(vert);
        if (laser_ring)
        {
            int rank = 0; // lasers below this one: a smaller angle, or an equal angle at a lower index
            for (int j = 0; j < n; j++)
            {
                const float other = (float) vert_correction_rad[j];
                rank += other < vert || (other == vert && j < i);
            }
            laser_ring[i] = rank;
        }
    }
    return CC_OK;
}

int cc_velodyne_create(cc_velodyne** out, int device, int num_streams, int max_packets, void* hip_stream)
{
    if (!out)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_create: null output handle");
    *out = nullptr;
    if (num_streams <= 0 || max_packets <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_create: num_streams and max_packets must be positive");
    if (num_streams > 65535)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_create: at most 65535 streams (the grid's second dimension)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(CC_ERR_NO_DEVICE, "cc_velodyne_create: no gfx950 device (there is no CPU variant of this path)");
    VELODYNE_HIP_CHECK(hipSetDevice(device));
    cc_velodyne* o = new cc_velodyne;
    o->device = device;
    o->num_streams = num_streams;
    o->max_packets = max_packets;
    o->stream_entry.assign(num_streams, -1);
    if (hip_stream)
        o->stream = (hipStream_t) hip_stream;
    else
    {
        VELODYNE_HIP_CHECK(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
        o->own_stream = true;
    }
    std::vector<float> tables(2 * ROTATION_MAX);
    rotation_tables(tables.data(), tables.data() + ROTATION_MAX);
    VELODYNE_HIP_CHECK(hipMalloc(&o->d_tables, tables.size() * sizeof(float)));
    VELODYNE_HIP_CHECK(hipMemcpy(o->d_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice));
    VELODYNE_HIP_CHECK(hipMalloc(&o->d_cals, (size_t) num_streams * sizeof(StreamCal)));
    VELODYNE_HIP_CHECK(hipMemset(o->d_cals, 0, (size_t) num_streams * sizeof(StreamCal)));
    VELODYNE_HIP_CHECK(hipMalloc(&o->d_counters, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    VELODYNE_HIP_CHECK(hipMemset(o->d_counters, 0, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    *out = o;
    return CC_OK;
}

void cc_velodyne_destroy(cc_velodyne* o)
{
    if (!o)
        return;
    (void) hipSetDevice(o->device);
    (void) hipStreamSynchronize(o->stream);
    for (CalEntry& e : o->entries)
        if (e.d)
            (void) hipFree(e.d);
    if (o->d_tables)
        (void) hipFree(o->d_tables);
    if (o->d_cals)
        (void) hipFree(o->d_cals);
    if (o->d_counters)
        (void) hipFree(o->d_counters);
    if (o->own_stream)
        (void) hipStreamDestroy(o->stream);
    delete o;
}

void* cc_velodyne_hip_stream(cc_velodyne* o)
{
    return o ? (void*) o->stream : nullptr;
}

int cc_velodyne_sync(cc_velodyne* o)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    VELODYNE_HIP_CHECK(hipSetDevice(o->device));
    VELODYNE_HIP_CHECK(hipStreamSynchronize(o->stream));
    return CC_OK;
}

int cc_velodyne_set_calibration(cc_velodyne* o, int stream, const float* cos_rot_correction, const float* sin_rot_correction,
                                const float* cos_vert_correction, const float* sin_vert_correction, const int32_t* laser_ring)
{
    // the arrays are judged first, so that a bad calibration is refused with its own text whatever else is wrong
    if (!cos_rot_correction || !sin_rot_correction || !cos_vert_correction || !sin_vert_correction || !laser_ring)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_set_calibration: all five arrays are required");
    unsigned char laser_of_row[ROWS];
    bool seen[ROWS] = {};
    for (int L = 0; L < ROWS; L++)
    {
        const int32_t ring = laser_ring[L];
        if (ring < 0 || ring >= ROWS || seen[ring])
            return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_set_calibration: laser_ring is not a permutation of 0..127 (laser " +
                                                     std::to_string(L) + " has ring " + std::to_string(ring) + ")");
        seen[ring] = true;
        laser_of_row[ROWS - 1 - ring] = (unsigned char) L; // row = 127 - ring (velodyne_input.hpp:55)
    }
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    if (stream < -1 || stream >= o->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_set_calibration: no stream " + std::to_string(stream));
    std::vector<float> trig(4 * ROWS);
    for (int L = 0; L < ROWS; L++)
    {
        trig[4 * L + 0] = cos_rot_correction[L];
        trig[4 * L + 1] = sin_rot_correction[L];
        trig[4 * L + 2] = cos_vert_correction[L];
        trig[4 * L + 3] = sin_vert_correction[L];
    }
    VELODYNE_HIP_CHECK(hipSetDevice(o->device));
    int idx = -1;
    for (size_t i = 0; i < o->entries.size() && idx < 0; i++)
    {
        const CalEntry& e = o->entries[i];
        if (e.d && !std::memcmp(e.trig.data(), trig.data(), trig.size() * sizeof(float)) &&
            !std::memcmp(e.ring.data(), laser_ring, ROWS * sizeof(int32_t)))
            idx = (int) i;
    }
    // kernels in flight may read the table (and an entry about to be released)
    VELODYNE_HIP_CHECK(hipStreamSynchronize(o->stream));
    if (idx < 0)
    {
        CalEntry e;
        e.trig = trig;
        e.ring.assign(laser_ring, laser_ring + ROWS);
        std::vector<unsigned char> image(CAL_DEVICE_BYTES);
        std::memcpy(image.data(), trig.data(), ROWS * sizeof(float4));
        std::memcpy(image.data() + ROWS * sizeof(float4), laser_of_row, ROWS);
        VELODYNE_HIP_CHECK(hipMalloc(&e.d, CAL_DEVICE_BYTES));
        VELODYNE_HIP_CHECK(hipMemcpy(e.d, image.data(), CAL_DEVICE_BYTES, hipMemcpyHostToDevice));
        o->entries.push_back(std::move(e));
        idx = (int) o->entries.size() - 1;
    }
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? o->num_streams : stream + 1;
    for (int s = s0; s < s1; s++)
    {
        const int old = o->stream_entry[s];
        o->entries[idx].refs++;
        if (old >= 0)
            o->entries[old].refs--;
        o->stream_entry[s] = idx;
    }
    for (CalEntry& e : o->entries)
        if (e.d && e.refs == 0)
        {
            VELODYNE_HIP_CHECK(hipFree(e.d));
            e.d = nullptr;
            e.trig.clear();
            e.ring.clear();
        }
    std::vector<StreamCal> table(o->num_streams, StreamCal{nullptr, nullptr});
    for (int s = 0; s < o->num_streams; s++)
        if (o->stream_entry[s] >= 0)
        {
            const CalEntry& e = o->entries[o->stream_entry[s]];
            table[s] = StreamCal{(const float4*) e.d, e.d + ROWS * sizeof(float4)};
        }
    VELODYNE_HIP_CHECK(hipMemcpy(o->d_cals, table.data(), table.size() * sizeof(StreamCal), hipMemcpyHostToDevice));
    return CC_OK;
}

int cc_velodyne_decode(cc_velodyne* o, int n_packets, const uint8_t* d_packets, int64_t packet_stride, const double* d_packet_poses,
                       const uint8_t* d_skip, float* d_xyz, uint8_t* d_intensity, double* d_poses, int32_t* d_block_azimuth)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    if (n_packets < 0 || n_packets > o->max_packets)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_decode: n_packets " + std::to_string(n_packets) + " not in 0..max_packets (" +
                                                 std::to_string(o->max_packets) + ")");
    for (int s = 0; s < o->num_streams; s++)
        if (o->stream_entry[s] < 0)
            return fail(CC_ERR_INVALID_ARGUMENT,
                        "cc_velodyne_decode: stream " + std::to_string(s) + " has no calibration (cc_velodyne_set_calibration)");
    if (packet_stride < PACKET_BYTES || packet_stride % 2 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_decode: packet_stride must be an even number of bytes >= 1206");
    if (n_packets == 0)
        return CC_OK;
    if (!d_packets || !d_xyz || !d_intensity || (d_packet_poses && !d_poses))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_decode: d_packets, d_xyz, d_intensity (and d_poses with d_packet_poses) are required");
    auto misaligned = [](const void* p, uintptr_t a) { return p && ((uintptr_t) p % a) != 0; };
    if (misaligned(d_packets, 2) || misaligned(d_xyz, 16) || misaligned(d_intensity, 4) || misaligned(d_poses, 16) ||
        misaligned(d_packet_poses, 16) || misaligned(d_block_azimuth, 4))
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_velodyne_decode: misaligned buffer (packets 2 B, xyz / poses / packet poses 16 B, intensity / block azimuth 4 B)");
    VELODYNE_HIP_CHECK(hipSetDevice(o->device));
    DecodeArgs a;
    a.packets = d_packets;
    a.packet_poses = d_packet_poses;
    a.skip = d_skip;
    a.xyz = d_xyz;
    a.intensity = d_intensity;
    a.poses = d_poses;
    a.block_azimuth = d_block_azimuth;
    a.cals = o->d_cals;
    a.cos_tab = o->d_tables;
    a.sin_tab = o->d_tables + ROTATION_MAX;
    a.counters = o->d_counters;
    a.stride = packet_stride;
    a.n_packets = n_packets;
    const uintptr_t both = (uintptr_t) d_packets | (uintptr_t) packet_stride;
    a.load_bytes = both % 16 == 0 ? 16 : both % 4 == 0 ? 4 : 2;
    const int groups = (n_packets + PACKETS_PER_WG - 1) / PACKETS_PER_WG;
    hipLaunchKernelGGL(k_velodyne_decode, dim3(groups, o->num_streams), dim3(BLOCK), 0, o->stream, a);
    VELODYNE_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_velodyne_counters(cc_velodyne* o, int stream, uint64_t* bad_block_header, uint64_t* dual_return_packets, uint64_t* skipped_packets)
{
    if (!o || stream < 0 || stream >= o->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_counters: no such stream");
    VELODYNE_HIP_CHECK(hipSetDevice(o->device));
    VELODYNE_HIP_CHECK(hipStreamSynchronize(o->stream));
    unsigned long long v[NUM_COUNTERS];
    VELODYNE_HIP_CHECK(hipMemcpy(v, o->d_counters + (size_t) stream * NUM_COUNTERS, sizeof(v), hipMemcpyDeviceToHost));
    if (bad_block_header)
        *bad_block_header = v[CNT_BAD_HEADER];
    if (dual_return_packets)
        *dual_return_packets = v[CNT_DUAL];
    if (skipped_packets)
        *skipped_packets = v[CNT_SKIPPED];
    return CC_OK;
}

int cc_velodyne_check_engine(cc_velodyne* o, struct cc_engine* e)
{
    if (!o || !e)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_check_engine: null handle");
    cc_stream_state st;
    int rc = cc_engine_stream_state(e, o->num_streams - 1, &st);
    if (rc == CC_ERR_INVALID_ARGUMENT || (rc == CC_OK && cc_engine_stream_state(e, o->num_streams, &st) == CC_OK))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_velodyne_check_engine: the engine does not have " + std::to_string(o->num_streams) + " streams");
    if (rc != CC_OK)
        return fail(rc, std::string("cc_velodyne_check_engine: ") + cc_engine_last_error(e));
    if (st.num_rows != ROWS)
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_velodyne_check_engine: the decoder has " + std::to_string(ROWS) + " rows, the engine " + std::to_string(st.num_rows));
    return CC_OK;
}

} // extern "C"
