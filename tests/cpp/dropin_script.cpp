// dropin_script.cpp — runs a script of operations on ONE continuous_clustering::ContinuousClustering object (the MI355X build) and dumps
// everything its callbacks and public members show, so that tests/test_gpu_dropin_scripts.py can compare it with the CPU oracle driven through
// the same operations. Where dropin_demo.cpp drives the class like kitti_demo.cpp does (one configuration, one reset, one stream), a script
// resets, reconfigures, changes the transform and the batching between firings, and goes on after an exception.
//
//   dropin_script <in.bin> <out.bin>
// in.bin : int32 magic 'DSC1', int32 number of operations, then per operation an int32 code and its arguments:
//   1 CONFIG    33 doubles, the fields of cc_config in the order of FIELDS below        -> setConfiguration
//   2 RESET     int32 rows                                                             -> reset
//   3 TRANSFORM 12 doubles                                                             -> setTransformRobotFrameFromSensorFrame
//   4 BATCH     int32 b: > 0 setBatchSize(b), 0 setAdaptiveBatching()
//   5 FLUSH                                                                            -> flush
//   6 FIRINGS   int32 n, rows, segment, first; n*rows*3 float xyz, n*rows uint8 intensity, n*12 double poses -> addFiring each
//               firing k = first + i: stamp 1e6 + 45 k, globally_unique_point_index (segment << 48) | (k << 16) | row
//   7 QUERY
// out.bin: records, each an int32 tag and a body (writers below); one record is written in one piece under a mutex, because in the asynchronous
// mode the callbacks run on the class's worker thread.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../continuous_clustering_amd/csrc/continuous_clustering.hpp"

using namespace continuous_clustering;

namespace
{
// ---- the configuration, restated: position in the CONFIG record -> member of Configuration ------------------------------------------------
const char* const FIELDS[33] = {"is_single_threaded",
                                "sensor_is_clockwise",
                                "num_columns",
                                "supplement_inclination_angle_for_nan_cells",
                                "max_slope",
                                "first_ring_as_ground_max_allowed_z_diff",
                                "first_ring_as_ground_min_allowed_z_diff",
                                "last_ground_point_slope_higher_than",
                                "last_ground_point_distance_smaller_than",
                                "ground_because_close_to_last_certain_ground_max_z_diff",
                                "ground_because_close_to_last_certain_ground_max_dist_diff",
                                "obstacle_because_next_certain_obstacle_max_dist_diff",
                                "use_terrain",
                                "terrain_max_allowed_z_diff",
                                "height_ref_to_maximum_",
                                "height_ref_to_ground_",
                                "length_ref_to_front_end_",
                                "length_ref_to_rear_end_",
                                "width_ref_to_left_mirror_",
                                "width_ref_to_right_mirror_",
                                "fog_filtering_enabled",
                                "fog_filtering_intensity_below",
                                "fog_filtering_distance_below",
                                "fog_filtering_inclination_above",
                                "max_distance",
                                "max_steps_in_row",
                                "max_steps_in_column",
                                "stop_after_association_enabled",
                                "stop_after_association_min_steps",
                                "ignore_points_in_chessboard_pattern",
                                "ignore_points_with_too_big_inclination_angle_diff",
                                "use_last_point_for_cluster_stamp",
                                "cluster_point_trees_every_nth_column"};

void fillConfiguration(const double v[33], Configuration& c)
{
    int i = 0;
    c.general.is_single_threaded = v[i++] != 0;
    auto& ri = c.range_image;
    ri.sensor_is_clockwise = v[i++] != 0;
    ri.num_columns = static_cast<int>(v[i++]);
    ri.supplement_inclination_angle_for_nan_cells = v[i++] != 0;
    auto& g = c.ground_segmentation;
    g.max_slope = static_cast<float>(v[i++]);
    g.first_ring_as_ground_max_allowed_z_diff = static_cast<float>(v[i++]);
    g.first_ring_as_ground_min_allowed_z_diff = static_cast<float>(v[i++]);
    g.last_ground_point_slope_higher_than = static_cast<float>(v[i++]);
    g.last_ground_point_distance_smaller_than = static_cast<float>(v[i++]);
    g.ground_because_close_to_last_certain_ground_max_z_diff = static_cast<float>(v[i++]);
    g.ground_because_close_to_last_certain_ground_max_dist_diff = static_cast<float>(v[i++]);
    g.obstacle_because_next_certain_obstacle_max_dist_diff = static_cast<float>(v[i++]);
    g.use_terrain = v[i++] != 0;
    g.terrain_max_allowed_z_diff = static_cast<float>(v[i++]);
    g.height_ref_to_maximum_ = static_cast<float>(v[i++]);
    g.height_ref_to_ground_ = static_cast<float>(v[i++]);
    g.length_ref_to_front_end_ = static_cast<float>(v[i++]);
    g.length_ref_to_rear_end_ = static_cast<float>(v[i++]);
    g.width_ref_to_left_mirror_ = static_cast<float>(v[i++]);
    g.width_ref_to_right_mirror_ = static_cast<float>(v[i++]);
    g.fog_filtering_enabled = v[i++] != 0;
    g.fog_filtering_intensity_below = static_cast<uint8_t>(v[i++]);
    g.fog_filtering_distance_below = static_cast<float>(v[i++]);
    g.fog_filtering_inclination_above = static_cast<float>(v[i++]);
    auto& k = c.clustering;
    k.max_distance = static_cast<float>(v[i++]);
    k.max_steps_in_row = static_cast<int>(v[i++]);
    k.max_steps_in_column = static_cast<int>(v[i++]);
    k.stop_after_association_enabled = v[i++] != 0;
    k.stop_after_association_min_steps = static_cast<int>(v[i++]);
    k.ignore_points_in_chessboard_pattern = v[i++] != 0;
    k.ignore_points_with_too_big_inclination_angle_diff = v[i++] != 0;
    k.use_last_point_for_cluster_stamp = v[i++] != 0;
    k.cluster_point_trees_every_nth_column = static_cast<int>(v[i++]);
    if (i != 33 || std::string(FIELDS[32]) != "cluster_point_trees_every_nth_column")
        abort();
}

// ---- records --------------------------------------------------------------------------------------------------------------------------------
#pragma pack(push, 1)
struct PublishedCell // tag 1, per cell of the range; behind all cells the child lists, then the associated-tree lists, one after the other
{
    uint64_t id, globally_unique_point_index, stamp, firing_index, tree_id;
    int64_t global_column_index, tree_root_column;
    double continuous_azimuth_angle, finished_at_continuous_azimuth_angle;
    float xyz[3], distance, inclination_angle, azimuth_angle;
    int32_t local_column_index, row_index, tree_root_row, number_of_visited_neighbors;
    uint32_t tree_num_points, cluster_width, n_child_points, n_associated_trees;
    uint8_t ground_point_label, debug_ground_point_label, is_ignored, intensity, belongs_to_finished_cluster;
};
struct ListEntry
{
    int64_t column_index;
    int32_t row_index;
};
struct GroundCell // tag 4, per cell of the column
{
    uint64_t globally_unique_point_index, stamp, firing_index;
    int64_t global_column_index;
    float xyz[3], distance, inclination_angle, azimuth_angle;
    int32_t row_index;
    uint8_t ground_point_label, debug_ground_point_label, is_ignored, intensity;
};
struct ClusterMember // tag 2, per point of the vector
{
    uint64_t id, stamp, globally_unique_point_index;
    int64_t global_column_index;
    int32_t row_index;
};
#pragma pack(pop)
static_assert(sizeof(PublishedCell) == 133 && sizeof(ListEntry) == 12 && sizeof(GroundCell) == 64 && sizeof(ClusterMember) == 36, "record layout");

struct Writer
{
    FILE* out{nullptr};
    std::mutex mu;
    void put(int32_t tag, const std::vector<char>& body)
    {
        std::lock_guard<std::mutex> lk(mu);
        fwrite(&tag, 4, 1, out);
        if (!body.empty())
            fwrite(body.data(), 1, body.size(), out);
    }
};

template<class T>
void add(std::vector<char>& b, const T& v)
{
    const char* p = reinterpret_cast<const char*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}

template<class T>
bool take(FILE* f, T* v, size_t n = 1)
{
    return fread(v, sizeof(T), n, f) == n;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 3)
        return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    int32_t hdr[2];
    if (!take(f, hdr, 2) || hdr[0] != 0x31435344)
        return 2;
    Writer w;
    w.out = fopen(argv[2], "wb");
    if (!w.out)
        return 2;

    ContinuousClustering clustering;
    long long n_ground_cb = 0, n_cluster_cb = 0, n_ground_view_violations = 0;
    clustering.setFinishedColumnCallback(
        [&](int64_t from, int64_t to, bool ground_points_only)
        {
            const int R = clustering.num_rows_;
            std::vector<char> b;
            add(b, from);
            add(b, to);
            if (ground_points_only)
            {
                n_ground_cb++;
                const int lc = static_cast<int>(from % clustering.ring_buffer_max_columns);
                for (int r = 0; r < R; r++)
                {
                    const Point& p = clustering.range_image_[(size_t) lc * R + r];
                    // the ground view runs before the column is associated (cc.cpp:618-623): clustering fields still as clearColumns left them
                    if (p.global_column_index != from || p.tree_root_.column_index != -1 || p.id != 0 || !p.child_points.empty() ||
                        p.number_of_visited_neighbors != 0 || p.ground_point_label == 0)
                        n_ground_view_violations++;
                    GroundCell c{};
                    c.globally_unique_point_index = p.globally_unique_point_index;
                    c.stamp = p.stamp;
                    c.firing_index = p.firing_index;
                    c.global_column_index = p.global_column_index;
                    c.xyz[0] = p.xyz.x, c.xyz[1] = p.xyz.y, c.xyz[2] = p.xyz.z;
                    c.distance = p.distance;
                    c.inclination_angle = p.inclination_angle;
                    c.azimuth_angle = p.azimuth_angle;
                    c.row_index = p.row_index;
                    c.ground_point_label = p.ground_point_label;
                    c.debug_ground_point_label = p.debug_ground_point_label;
                    c.is_ignored = p.is_ignored;
                    c.intensity = p.intensity;
                    add(b, c);
                }
                w.put(4, b);
                return;
            }
            std::vector<ListEntry> children, trees;
            for (int64_t g = from; g <= to; g++)
            {
                const int lc = static_cast<int>(g % clustering.ring_buffer_max_columns);
                for (int r = 0; r < R; r++)
                {
                    const Point& p = clustering.range_image_[(size_t) lc * R + r];
                    PublishedCell c{};
                    c.id = p.id;
                    c.globally_unique_point_index = p.globally_unique_point_index;
                    c.stamp = p.stamp;
                    c.firing_index = p.firing_index;
                    c.tree_id = p.tree_id;
                    c.global_column_index = p.global_column_index;
                    c.tree_root_column = p.tree_root_.column_index;
                    c.continuous_azimuth_angle = p.continuous_azimuth_angle;
                    c.finished_at_continuous_azimuth_angle = p.finished_at_continuous_azimuth_angle;
                    c.xyz[0] = p.xyz.x, c.xyz[1] = p.xyz.y, c.xyz[2] = p.xyz.z;
                    c.distance = p.distance;
                    c.inclination_angle = p.inclination_angle;
                    c.azimuth_angle = p.azimuth_angle;
                    c.local_column_index = p.local_column_index;
                    c.row_index = p.row_index;
                    c.tree_root_row = p.tree_root_.row_index;
                    c.number_of_visited_neighbors = p.number_of_visited_neighbors;
                    c.tree_num_points = p.tree_num_points;
                    c.cluster_width = p.cluster_width;
                    c.n_child_points = static_cast<uint32_t>(p.child_points.size());
                    c.n_associated_trees = static_cast<uint32_t>(p.associated_trees.size());
                    c.ground_point_label = p.ground_point_label;
                    c.debug_ground_point_label = p.debug_ground_point_label;
                    c.is_ignored = p.is_ignored;
                    c.intensity = p.intensity;
                    c.belongs_to_finished_cluster = p.belongs_to_finished_cluster;
                    add(b, c);
                    for (const RangeImageIndex& ch : p.child_points)
                        children.push_back({ch.column_index, ch.row_index});
                    for (const RangeImageIndex& t : p.associated_trees) // (a std::set: sorted by row, then column)
                        trees.push_back({t.column_index, t.row_index});
                }
            }
            for (const ListEntry& e : children)
                add(b, e);
            for (const ListEntry& e : trees)
                add(b, e);
            w.put(1, b);
        });
    clustering.setFinishedClusterCallback(
        [&](const std::vector<Point>& pts, uint64_t stamp)
        {
            n_cluster_cb++;
            std::vector<char> b;
            const uint64_t cnt = pts.size();
            add(b, cnt);
            add(b, stamp);
            for (const Point& p : pts)
            {
                ClusterMember m{};
                m.id = p.id;
                m.stamp = p.stamp;
                m.globally_unique_point_index = p.globally_unique_point_index;
                m.global_column_index = p.global_column_index;
                m.row_index = p.row_index;
                add(b, m);
            }
            w.put(2, b);
        });

    auto exception_record = [&](int32_t op, int64_t firing, const char* what)
    {
        std::vector<char> b;
        const int32_t len = static_cast<int32_t>(strlen(what));
        add(b, op);
        add(b, firing);
        add(b, len);
        b.insert(b.end(), what, what + len);
        w.put(6, b);
    };

    for (int32_t op = 0; op < hdr[1]; op++)
    {
        int32_t code = 0;
        if (!take(f, &code))
            return 2;
        try
        {
            switch (code)
            {
                case 1:
                {
                    double v[33];
                    if (!take(f, v, 33))
                        return 2;
                    Configuration config;
                    fillConfiguration(v, config);
                    clustering.setConfiguration(config);
                    break;
                }
                case 2:
                {
                    int32_t rows;
                    if (!take(f, &rows))
                        return 2;
                    clustering.reset(rows);
                    break;
                }
                case 3:
                {
                    Pose3d tf;
                    if (!take(f, tf.m, 12))
                        return 2;
                    clustering.setTransformRobotFrameFromSensorFrame(tf);
                    break;
                }
                case 4:
                {
                    int32_t b;
                    if (!take(f, &b))
                        return 2;
                    if (b > 0)
                        clustering.setBatchSize(b);
                    else
                        clustering.setAdaptiveBatching();
                    break;
                }
                case 5:
                    clustering.flush();
                    break;
                case 6:
                {
                    int32_t a[4];
                    if (!take(f, a, 4))
                        return 2;
                    const int n = a[0], rows = a[1];
                    const uint64_t segment = static_cast<uint64_t>(a[2]), first = static_cast<uint64_t>(a[3]);
                    std::vector<float> xyz((size_t) n * rows * 3);
                    std::vector<uint8_t> inten((size_t) n * rows);
                    std::vector<double> poses((size_t) n * 12);
                    if (!take(f, xyz.data(), xyz.size()) || !take(f, inten.data(), inten.size()) || !take(f, poses.data(), poses.size()))
                        return 2;
                    for (int i = 0; i < n; i++)
                    {
                        const uint64_t k = first + static_cast<uint64_t>(i);
                        RawPoints::Ptr firing(new RawPoints);
                        firing->stamp = 1000000ull + 45ull * k;
                        firing->points.resize(rows);
                        for (int r = 0; r < rows; r++)
                        {
                            RawPoint& q = firing->points[r];
                            q.x = xyz[((size_t) i * rows + r) * 3 + 0];
                            q.y = xyz[((size_t) i * rows + r) * 3 + 1];
                            q.z = xyz[((size_t) i * rows + r) * 3 + 2];
                            q.intensity = inten[(size_t) i * rows + r];
                            q.stamp = firing->stamp;
                            q.firing_index = k;
                            q.globally_unique_point_index = (segment << 48) | (k << 16) | (uint64_t) r;
                        }
                        Pose3d pose;
                        for (int j = 0; j < 12; j++)
                            pose.m[j] = poses[(size_t) i * 12 + j];
                        try
                        {
                            clustering.addFiring(firing, pose);
                        }
                        catch (const std::exception& e)
                        {
                            exception_record(op, static_cast<int64_t>(k), e.what());
                            break; // the rest of this operation's firings is not fed; the script goes on with the next operation
                        }
                    }
                    break;
                }
                case 7:
                {
                    std::vector<char> b;
                    const int32_t q[5] = {clustering.resetRequired() ? 1 : 0, clustering.hasTransformRobotFrameFromSensorFrame() ? 1 : 0, clustering.num_rows_,
                                          clustering.num_columns_, clustering.ring_buffer_max_columns};
                    add(b, op);
                    add(b, q);
                    add(b, clustering.ring_buffer_start_global_column_index);
                    add(b, clustering.ring_buffer_end_global_column_index);
                    w.put(5, b);
                    break;
                }
                default:
                    return 2;
            }
        }
        catch (const std::exception& e)
        {
            exception_record(op, -1, e.what());
        }
        // "operation done": what was written before this record was caused by this operation or, in the asynchronous mode, by firings of earlier ones
        std::vector<char> b;
        add(b, op);
        add(b, code);
        w.put(7, b);
    }
    fclose(f);
    try
    {
        clustering.flush();
    }
    catch (const std::exception& e)
    {
        exception_record(hdr[1], -1, e.what());
    }
    std::vector<char> b;
    add(b, n_ground_cb);
    add(b, n_cluster_cb);
    add(b, n_ground_view_violations);
    w.put(3, b);
    fclose(w.out);
    printf("ok ground_cb=%lld cluster_cb=%lld\n", n_ground_cb, n_cluster_cb);
    return 0;
}
