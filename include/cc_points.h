/* cc_points.h — C-ABI of the generic PointCloud2 decoder that sits immediately upstream of insertion.
 *
 * The reference's third input, GenericPointsInput (ros/generic_points_input.hpp:21-53, sensor_manufacturer "generic_points",
 * src/ros/continuous_clustering_node.cpp:41-46), takes one sensor_msgs/PointCloud2 per firing: height = number of lasers, width = 1,
 * and reads the fields "x", "y", "z" and "intensity" of every point on a host thread. It is the input of every sensor without a
 * packet decoder, and the only one that reads back the firings the node itself publishes (firingToPointCloud,
 * src/ros/ros_utils.cpp:79-106). This library does that decode as a HIP kernel on gfx950 and writes the firings straight into the
 * arrays cc_engine_add_firings_device (cc_hip.h) consumes, so the message bytes go to HBM once and never come back to the host. There
 * is no CPU variant of the device path: cc_points_create fails with CC_ERR_NO_DEVICE without a GPU. The message layout is not fixed by
 * a sensor: it is the run-time description cc_points_layout below, with arbitrary byte offsets and strides. Not handled: unorganised
 * clouds (nothing maps a point to a row and a column), big-endian messages, per-point time fields.
 *
 * ---- UNPINNED: the field access below restates sensor_msgs::PointCloud2ConstIterator (sensor_msgs/point_cloud2_iterator.h) as the
 * ---- reference uses it, without that header (ROS is not a dependency and is not available to check against).
 *
 * Message: a blob of message_bytes bytes. Point (row r, column c) starts at byte r * row_stride + c * column_stride; a PointCloud2 has
 * row_stride = row_step and column_stride = point_step (with width 1, row_step == point_step). The iterator of field "x" is a pointer
 * to byte `offset of x` of the first point that advances by point_step and is dereferenced as its template type, whatever the
 * field's declared datatype: the datatype is not consulted. Hence:
 *
 *   xyz        the four bytes at off_x / off_y / off_z of the point, little-endian, copied bit for bit (generic_points_input.hpp:32-34,
 *              43-45): NaN payloads, -0.0, infinities and denormals arrive unchanged. A NaN x is "no return", as everywhere in the engine.
 *   intensity  by intensity_mode, from the field at off_intensity (off_intensity == -1: 0 everywhere):
 *     CC_POINTS_INTENSITY_REFERENCE  the reference reads the field through PointCloud2ConstIterator<uint8_t> and stores
 *                                    static_cast<uint8_t>(*it * 255) (:35, :46). *it is the FIRST BYTE b of the field, the product is
 *                                    an int, so the result is (b * 255) & 0xFF (== (256 - b) & 0xFF: 0 -> 0, 1 -> 255, 255 -> 1). With
 *                                    the UINT8 field of the reference's own RAW_POINT message this is what the node computes; with a
 *                                    FLOAT32 intensity field the reference therefore yields a function of the float's LOW MANTISSA
 *                                    BYTE, not of its value.
 *     CC_POINTS_INTENSITY_U8         the byte verbatim.
 *     CC_POINTS_INTENSITY_F32_UNIT   an f32 v in [0, 1], converted as the KITTI path converts `i * 255` (kitti_demo.cpp:148,
 *                                    cc_kitti.hip): p = v * 255 in f32; p inside (-2^31, 2^31): the low byte of (int32) p (truncated
 *                                    toward zero, two's complement); otherwise (and NaN) 0.
 *     CC_POINTS_INTENSITY_F32_255    an f32 v on a 0..255 scale (what the common ROS lidar drivers publish): NaN -> 0, otherwise v
 *                                    clamped to [0, 255] and truncated.
 *   rows       message row r becomes engine row r (:37-48: row_index counts the points in message order), or H - 1 - r with reverse_rows.
 *
 * Beyond the reference (the one generalisation): a message may be an organised cloud of `columns` > 1 columns; column c of message m
 * becomes firing m * columns + c of its stream. The reference's message is columns == 1.
 *
 * Dropped messages: the reference returns from a message with a zero stamp (:23-24). The caller marks such a message (or the padding
 * of a stream that delivered nothing) in d_skip; every column of a marked message is written as an ALL-NaN firing with intensity 0
 * and the message is not read. An all-NaN firing changes nothing observable in the engine except firings_consumed and the
 * source_firing of a column view.
 *
 * All device arrays are [num_streams][...] with the stream stride implied by n_messages of the call, exactly the layout of
 * cc_engine_add_firings_device for n = n_messages * columns firings per stream. Functions return CC_OK (0) or a CC_ERR_* code of
 * cc_hip.h; cc_points_last_error() has the text.
 */
#ifndef CC_POINTS_H
#define CC_POINTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_points cc_points;

enum
{
    CC_POINTS_INTENSITY_REFERENCE = 0,
    CC_POINTS_INTENSITY_U8 = 1,
    CC_POINTS_INTENSITY_F32_UNIT = 2,
    CC_POINTS_INTENSITY_F32_255 = 3
};

typedef struct cc_points_layout {
    int32_t rows;            /* H: engine rows; a multiple of 4, 4..128 (as cc_ouster_create) */
    int32_t columns;         /* C >= 1: firings per message; the reference's case is 1 (width == 1) */
    int64_t row_stride;      /* bytes from row r to row r+1 of one column (PointCloud2: row_step; with width 1 == point_step) */
    int64_t column_stride;   /* bytes from column c to c+1 of one row   (PointCloud2: point_step) */
    int32_t off_x, off_y, off_z;   /* byte offset of each f32 inside a point, any alignment */
    int32_t off_intensity;   /* byte offset, or -1: intensity 0 everywhere */
    int32_t intensity_mode;  /* CC_POINTS_INTENSITY_* above */
    int32_t reverse_rows;    /* 0: message row r -> engine row r (generic_points_input.hpp:37-48); 1: -> H-1-r */
    int64_t message_bytes;   /* bytes of one message the decoder may read; every field of every (row, column) lies inside */
} cc_points_layout;

/* ---- host-only helpers (plain C, no device) ------------------------------------------------------------------------------- */

/* The validation cc_points_create applies. CC_ERR_INVALID_ARGUMENT with a text for: rows not a multiple of 4 or outside 4..128;
 * columns < 1; a stride <= 0; an unknown intensity mode; off_intensity < -1; any byte of x, y, z (4 bytes each) or of the intensity
 * field (1 byte in modes 0 and 1, 4 bytes in modes 2 and 3) of any (row, column) outside [0, message_bytes). */
int cc_points_layout_check(const cc_points_layout* layout);

/* How the kernel walks this layout (results never depend on it). cc_points_path: 2 = columns == 1, a workgroup stages the contiguous
 * field bytes of several whole messages; 1 = row-major organised cloud (column_stride < row_stride), a workgroup stages one row segment
 * per row for a tile of columns; 0 = anything else (or a layout whose staging would not fit in LDS): fields are gathered from global
 * memory byte by byte. cc_points_column_tile: firings one workgroup produces (columns of the tile on path 1, messages on path 2).
 * Both return -1 for a layout cc_points_layout_check refuses. */
int cc_points_path(const cc_points_layout* layout);
int cc_points_column_tile(const cc_points_layout* layout);

/* ---- device decode --------------------------------------------------------------------------------------------------------- */

/* One handle decodes num_streams streams that share `layout` (copied). max_messages: messages per stream one decode call may carry.
 * hip_stream: the hipStream_t the decode is enqueued on (pass cc_engine_hip_stream(e) and set the engine option
 * "input_on_engine_stream" to chain with an engine; destroy the decoder before that engine); NULL = own stream. */
int cc_points_create(cc_points** out, int device, int num_streams, const cc_points_layout* layout, int max_messages, void* hip_stream);
void cc_points_destroy(cc_points* o);
const char* cc_points_last_error(void);
void* cc_points_hip_stream(cc_points* o);
int cc_points_sync(cc_points* o);

/* Check that the firings of this decoder fit engine `e` (include cc_hip.h first): same number of streams, engine rows == layout.rows.
 * CC_ERR_INVALID_ARGUMENT with a cc_points_last_error text otherwise. Synchronises the engine; call it once when pairing the two. */
struct cc_engine;
int cc_points_check_engine(cc_points* o, struct cc_engine* e);

/* Decode n_messages messages of every stream (asynchronous, on the handle's HIP stream), 1 <= n_messages <= max_messages. The byte
 * address of point (row r, column c) of message m of stream s is
 *     d_messages + (s * n_messages + m) * message_stride + r * row_stride + c * column_stride.
 * DEVICE pointers:
 *   d_messages        uint8, ANY byte alignment; message_stride >= message_bytes, any value (a PointCloud2 blob lands wherever its
 *                     transport put it). The kernel reads nothing outside [d_messages, d_messages + S * n_messages * message_stride).
 *   d_message_poses   [S][n_messages][12] doubles   odom_from_sensor of each message, replicated to its `columns` firings; NULL =
 *                                                   d_poses is left as the caller wrote it (16-byte aligned)
 *   d_skip            [S][n_messages] uint8         nonzero: every column of the message becomes an all-NaN firing with intensity 0
 *                                                   (the message is not read); NULL = none
 *   d_xyz             [S][n_messages * C][H][3] float  (16-byte aligned)
 *   d_intensity       [S][n_messages * C][H] uint8     (4-byte aligned)
 *   d_poses           [S][n_messages * C][12] double   (16-byte aligned; may be NULL only with d_message_poses NULL)
 * CC_ERR_INVALID_ARGUMENT with a text (nothing is launched) for n_messages outside 1..max_messages, message_stride < message_bytes,
 * a missing d_messages / d_xyz / d_intensity (or d_poses with d_message_poses), a misaligned output or pose array. */
int cc_points_decode(cc_points* o, int n_messages, const uint8_t* d_messages, int64_t message_stride, const double* d_message_poses,
                     const uint8_t* d_skip, float* d_xyz, uint8_t* d_intensity, double* d_poses);

/* Since create, per stream (synchronises). skipped_messages: messages marked in d_skip (a message counts once, whatever its columns);
 * no_return_points: points with a NaN x in the messages that were decoded (the placeholders of a skipped message are not counted).
 * Either pointer may be NULL. */
int cc_points_counters(cc_points* o, int stream, uint64_t* skipped_messages, uint64_t* no_return_points);

#ifdef __cplusplus
}
#endif
#endif
