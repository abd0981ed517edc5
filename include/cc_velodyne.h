/* cc_velodyne.h — C-ABI of the Velodyne VLS-128 packet decoder that sits immediately upstream of insertion.
 *
 * The reference's live Velodyne front end (VelodyneInput, ros/velodyne_input.hpp:46-91) hands every UDP payload to the ROS driver's
 * RawData::unpack_vls128 on a host thread and collects one 128-row firing per firing sequence. This library does that decode as a HIP
 * kernel on gfx950 and writes the firings straight into the arrays cc_engine_add_firings_device (cc_hip.h) consumes, so packets go to
 * HBM once and never come back to the host. There is no CPU variant of the device path: cc_velodyne_create fails with
 * CC_ERR_NO_DEVICE without a GPU. The VLS-128 is the one Velodyne the reference names as tested (launch/sensor_vls128_roof.launch);
 * other models, dual-return decode and the position packet are not handled.
 *
 * ---- UNPINNED: everything from here to the end of this comment is restated from ros-drivers/velodyne RawData::unpack_vls128 and
 * ---- velodyne_pointcloud::Calibration without that driver (it is not a dependency and no recording is available to check against).
 *
 * Packet (little-endian, 1206 bytes): 12 blocks of 100 bytes, then u32 timestamp @1200, u8 return mode @1204, u8 model @1205.
 *
 *     offset in block           field
 *     0                         u16 header: bank 0xEEFF / 0xDDFF / 0xCCFF / 0xBBFF = lasers 0-31 / 32-63 / 64-95 / 96-127
 *     2                         u16 rotation, 0.01 degree
 *     4 + 3*j + 0               u16 distance of laser j + 32*bank, 0.004 m
 *     4 + 3*j + 2               u8  intensity
 *
 * Firing slot f (0..2) of a packet is blocks 4f .. 4f+3 and becomes firing 3p + f of its stream. A slot is valid iff its four headers
 * are banks 0xEEFF, 0xDDFF, 0xCCFF, 0xBBFF in this order and every earlier slot of the packet is valid (the driver returns from the
 * packet at the first bad header, and newLine() publishes only behind the fourth bank).
 *
 * Azimuth (C int arithmetic, % truncating toward zero; b = block in the packet):
 *     az[b] = rotation[b];  diff[b] = (float) ((36000 + rotation[b+1] - rotation[b]) % 36000) for b < 11, diff[11] = 0
 * Laser L = j + 32*bank, order = L / 8, frac[i] = (2.665f / 53.3f) * (float) (i + i / 8) for i = 0..15 (f32):
 *     a_f = (float) az + diff * frac[order]              (f32, two roundings, no FMA)
 *     a   = ((int32) round-half-away(a_f) & 0xFFFF) % 36000
 * The driver writes (uint16_t) round(a_f) % 36000; the cast of a value above 65535 (a rotation word >= 36000 can produce one) is
 * undefined behaviour, and what is written above is its x86-64 outcome (cvttss2si, then the low 16 bits). A rotation word >= 36000
 * also makes (36000 + next - this) negative, and % keeps the sign: diff is then negative, as in the driver.
 *
 * Rotation tables, i = 0..35999: rad = (float) ((double) (0.01f * i) * M_PI / 180.0), cos_tab[i] = cosf(rad), sin_tab[i] = sinf(rad)
 * (host libm; cc_velodyne_rotation_tables returns them). Calibration per laser: cosf / sinf of (float) rot_correction and of
 * (float) vert_correction; laser_ring = rank of (float) vert_correction ascending, the lower laser index first among equals.
 *
 * Point of laser L (all f32, every product and sum rounded; crc / src / cvc / svc = the laser's calibration):
 *     d  = (float) raw * 0.004f
 *     cr = cos_tab[a]*crc + sin_tab[a]*src;   sr = sin_tab[a]*crc - cos_tab[a]*src
 *     xy = d*cvc;   x = xy*cr;   y = -(xy*sr);   z = d*svc;   intensity = the byte
 * raw == 0: xyz = NaN, intensity 0 (velodyne_input.hpp:62-75). The driver's 0 .. 300 m range window (parser.setParameters(0, 300, ..),
 * :29) never bites: the largest distance is 65535 * 0.004 m = 262.14 m. Row = 127 - laser_ring[L] (:55).
 *
 * Pose: the packet's pose is replicated to its 3 firings. (The reference adds static_cast<uint64_t>(time / 1e9) to the packet stamp
 * (:57), which is always 0: every point of a packet carries the packet's stamp, so a packet pose is what it effectively uses.)
 *
 * Placeholders: an invalid slot, every slot of a packet whose return-mode byte is 57 (dual return: refused, counted, not decoded) and
 * every slot of a packet marked in d_skip is written as an ALL-NaN firing (intensity 0, block azimuth -1). The reference drops such
 * firings; an all-NaN firing changes nothing observable in the engine, so labels, ids, events and published columns equal those of
 * the dropped stream. Only firings_consumed and the source_firing of a column view count the placeholders.
 *
 * All device arrays are [num_streams][...] with the stream stride implied by n_packets of the call, exactly the layout of
 * cc_engine_add_firings_device for n = 3 * n_packets firings per stream. Functions return CC_OK (0) or a CC_ERR_* code of cc_hip.h;
 * cc_velodyne_last_error() has the text.
 */
#ifndef CC_VELODYNE_H
#define CC_VELODYNE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_velodyne cc_velodyne;

/* max_packets: packets per stream one decode call may carry. hip_stream: the hipStream_t the decode is enqueued on (pass
 * cc_engine_hip_stream(e) and set the engine option "input_on_engine_stream" to chain with an engine; destroy the decoder before that
 * engine); NULL = own stream. */
int cc_velodyne_create(cc_velodyne** out, int device, int num_streams, int max_packets, void* hip_stream);
void cc_velodyne_destroy(cc_velodyne* o);
const char* cc_velodyne_last_error(void);
void* cc_velodyne_hip_stream(cc_velodyne* o);
int cc_velodyne_sync(cc_velodyne* o);

/* Fixed by the sensor: 128 and 3. */
int cc_velodyne_rows(void);
int cc_velodyne_firings_per_packet(void);

/* Check that the firings of this decoder fit engine `e` (include cc_hip.h first): same number of streams, engine rows == 128.
 * CC_ERR_INVALID_ARGUMENT with a cc_velodyne_last_error text otherwise. Synchronises the engine; call it once when pairing the two. */
struct cc_engine;
int cc_velodyne_check_engine(cc_velodyne* o, struct cc_engine* e);

/* The calibration of `stream` (-1 = all streams): host arrays of 128 entries indexed by laser (cc_velodyne_make_calibration writes
 * them). Streams given identical arrays share one device copy. A laser_ring that is not a permutation of 0..127 is refused. */
int cc_velodyne_set_calibration(cc_velodyne* o, int stream, const float* cos_rot_correction, const float* sin_rot_correction,
                                const float* cos_vert_correction, const float* sin_vert_correction, const int32_t* laser_ring);

/* Decode n_packets packets of every stream (asynchronous, on the handle's HIP stream). DEVICE pointers:
 *   d_packets         [S][n_packets][packet_stride] raw payloads; packet_stride >= 1206; base and stride at least 2-byte aligned (a real
 *                                                   payload is 1206 bytes, not a multiple of 4). Base and stride multiples of 16 let
 *                                                   the kernel stage with 16-B loads, multiples of 4 with dword loads.
 *   d_packet_poses    [S][n_packets][12] doubles    odom_from_sensor of each packet, replicated to its 3 firings; NULL = d_poses is left
 *                                                   as the caller wrote it (16-byte aligned)
 *   d_skip            [S][n_packets] uint8          nonzero: every slot of the packet becomes an all-NaN firing (the packet is not
 *                                                   read); NULL = none
 *   d_xyz             [S][3*n_packets][128][3] float  (16-byte aligned)
 *   d_intensity       [S][3*n_packets][128] uint8     (4-byte aligned)
 *   d_poses           [S][3*n_packets][12] double     (16-byte aligned; may be NULL only with d_packet_poses NULL)
 *   d_block_azimuth   [S][3*n_packets] int32          raw rotation word of the firing's first block, -1 for a placeholder; NULL = not wanted
 * Every stream needs a calibration (CC_ERR_INVALID_ARGUMENT otherwise). */
int cc_velodyne_decode(cc_velodyne* o, int n_packets, const uint8_t* d_packets, int64_t packet_stride, const double* d_packet_poses,
                       const uint8_t* d_skip, float* d_xyz, uint8_t* d_intensity, double* d_poses, int32_t* d_block_azimuth);

/* Placeholders since create, per stream (synchronises). bad_block_header: firing slots dropped for a block header (the slot with the
 * first wrong header and every later slot of its packet); dual_return_packets: packets refused for return mode 57; skipped_packets:
 * packets marked in d_skip. A skipped packet counts only as skipped, a dual-return packet only as dual. Any pointer may be NULL. */
int cc_velodyne_counters(cc_velodyne* o, int stream, uint64_t* bad_block_header, uint64_t* dual_return_packets, uint64_t* skipped_packets);

/* ---- host-only helpers (plain C, no device) ------------------------------------------------------------------------------- */

/* 1206. */
int64_t cc_velodyne_packet_bytes(void);

/* The rotation tables the kernel uses (formula above), 36000 floats each; either may be NULL. */
int cc_velodyne_rotation_tables(float* cos_table, float* sin_table);

/* The driver's per-laser angles (radians, laser index order, n = 128 for cc_velodyne_set_calibration) to the five arrays of
 * cc_velodyne_set_calibration (formula above). Any output may be NULL. */
int cc_velodyne_make_calibration(int n, const double* rot_correction_rad, const double* vert_correction_rad, float* cos_rot_correction,
                                 float* sin_rot_correction, float* cos_vert_correction, float* sin_vert_correction, int32_t* laser_ring);

#ifdef __cplusplus
}
#endif
#endif
