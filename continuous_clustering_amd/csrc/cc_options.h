// cc_options.h — the options of cc_engine_set_option (documented in include/cc_hip.h) as ONE table: name, kind, bounds, and what setting the
// option does to the engine. Host code only. Not a header of its own: cc_engine.hip includes it once, at the end of its anonymous namespace, behind
// everything the rows call (cc_engine, TREE_SLOTS, cck::SL_CAP, flush_deferred, finish_batch, forget_inclination_table, prewarm_small_calls).
// The names, kinds, bounds, the clamp and the look-up depend on nothing of that: a host-only program that defines CC_OPTIONS_TABLE_ONLY, declares
// cc_engine and supplies the two symbolic bounds gets them without HIP (tests/csrc/options_probe.cpp); its rows then carry no `apply`.
#include <stdint.h>
#include <string.h>

enum OptionKind
{
    OPT_BOOL,   // value != 0
    OPT_INT,    // clamped to [lo, hi]
    OPT_TRI,    // -1 (negative: automatic) / 0 / 1 (positive)
    OPT_ACTION, // nothing is stored: a value != 0 does something once
};

struct OptionDef
{
    const char* name;
    OptionKind kind;
    int64_t lo, hi;                      // what cc_option_clamp returns lies in [lo, hi]
    int (*apply)(cc_engine*, int64_t v); // stores the clamped value `v` and does what goes with it; CC_OK or an error code
};

// The value an option takes for a caller's `value`. The bounds are applied in 64 bits, before anything is narrowed to the field's type: a value beyond
// the 32-bit range saturates at the bound (where a row has no upper bound of its own, at INT32_MAX) and never wraps.
constexpr int64_t cc_option_clamp(const OptionDef& d, int64_t value)
{
    switch (d.kind)
    {
    case OPT_BOOL:
    case OPT_ACTION: return value != 0 ? 1 : 0;
    case OPT_TRI: return value < 0 ? -1 : (value != 0 ? 1 : 0);
    default: return value < d.lo ? d.lo : (value > d.hi ? d.hi : value);
    }
}

#ifdef CC_OPTIONS_TABLE_ONLY
#define CC_OPT_APPLY(...) nullptr
#else
#define CC_OPT_APPLY(...) [](cc_engine* e, int64_t v) -> int { __VA_ARGS__; return CC_OK; }
#endif
#define CC_OPT_BOOL(name_, ...) {name_, OPT_BOOL, 0, 1, CC_OPT_APPLY(__VA_ARGS__)}
#define CC_OPT_INT(name_, lo_, hi_, ...) {name_, OPT_INT, lo_, hi_, CC_OPT_APPLY(__VA_ARGS__)}
#define CC_OPT_TRI(name_, ...) {name_, OPT_TRI, -1, 1, CC_OPT_APPLY(__VA_ARGS__)}
#define CC_OPT_ACTION(name_, ...) {name_, OPT_ACTION, 0, 1, CC_OPT_APPLY(__VA_ARGS__)}

// One row per option, in the order of include/cc_hip.h. "pipeline" and "parallel_insert" start at -1 because a negative value has always meant
// "on, in the plain form" (as 1 and 2 respectively); "assoc_waves" ends at 5 because everything above 4 means automatic, like 0.
constexpr OptionDef CC_OPTIONS[] = {
    // -- pipeline shape of cc_engine_add_firings_device
    CC_OPT_INT("pipeline", -1, 2, e->allow_pipeline = v != 0, e->pipeline_depth = v >= 2 ? 2 : 1), // 0: one stream, 1: three chains, 2: four (window scan on its own stream)
    CC_OPT_INT("sub_batch", 0, INT64_MAX, e->sub_batch = v),
    CC_OPT_INT("limit_columns", 1, INT32_MAX, e->g.limit_columns = (int32_t) v),
    CC_OPT_BOOL("input_on_engine_stream", e->input_on_engine_stream = v != 0),
    CC_OPT_INT("defer_tail_max_streams", 0, INT32_MAX, e->defer_tail_max_streams = (int) v),
    CC_OPT_INT("lazy_gate", 0, 4096, int rc = flush_deferred(e); if (rc) return rc; e->lazy_gate_max_streams = (int) v, e->lazy_ok = true, e->lazy_miss = 0),
    CC_OPT_INT("lazy_gate_from", 0, 1 << 20, int rc = flush_deferred(e); if (rc) return rc; e->lazy_gate_from_streams = (int) v, e->lazy_ok = true, e->lazy_miss = 0),
    // -- insertion
    CC_OPT_INT("parallel_insert", -1, 2, e->parallel_insert = v != 0, e->parallel_insert_multi = v == 1),
    CC_OPT_BOOL("skip_idle_fallbacks", e->skip_idle_fallbacks = v != 0),
    CC_OPT_BOOL("fuse_front", e->fuse_front = v != 0),
    CC_OPT_INT("insert_wide_max_streams", 0, 1 << 20, e->insert_wide_max_streams = (int) v),
    CC_OPT_INT("insert_split_blocks", 0, 8, e->insert_split_blocks = (int) v),
    // -- segmentation, window scan
    CC_OPT_INT("seg_small_max", 0, 63, e->seg_small_max = (int) v, e->small_graphs_stale = true),
    CC_OPT_TRI("scan_packed", e->scan_packed = (int) v),
    CC_OPT_INT("scan_split", 0, 2, e->scan_split = (int) v),
    CC_OPT_INT("scan_cap", 1, 1 << 20, e->g.scan_cap = (int32_t) v),
    CC_OPT_TRI("scan_store_fin", e->scan_store_fin = (int) v),
    CC_OPT_INT("scan_long_records", 1, cck::SL_CAP, e->g.sl_cap = (int32_t) v),
    // -- association
    CC_OPT_BOOL("assoc_batch", e->assoc_batch = v != 0),
    CC_OPT_INT("assoc_rounds", 0, 8, e->assoc_rounds = (int) v),
    CC_OPT_INT("assoc_cooldown", 0, 1000, e->bail_cooldown_batches = (int) v),
    CC_OPT_INT("assoc_sweep_blocks", 1, 1024, e->assoc_sweep_blocks = (int) v),
    // 1: k_assoc_lds, 3: k_assoc3 without the links wave, 4: with it, 0 (default): k_assoc3, links wave up to 256 streams (2: as 3)
    CC_OPT_INT("assoc_waves", 0, 5, e->assoc_waves_auto = v <= 0 || v > 4, e->assoc_waves = e->assoc_waves_auto ? 3 : (int) v),
    CC_OPT_INT("lds_tree_limit", 1, TREE_SLOTS, e->g.lds_tree_limit = (int32_t) v),
    CC_OPT_BOOL("mirror_fields", e->g.mirror_fields = v != 0),
    // -- small calls of cc_engine_add_firings
    CC_OPT_BOOL("graphs", e->allow_graphs = v != 0),
    CC_OPT_BOOL("small_front", e->small_front = v != 0, e->small_graphs_stale = true),
    CC_OPT_BOOL("small_all", e->small_all = v != 0, e->small_graphs_stale = true),
    CC_OPT_BOOL("small_direct", e->small_direct = v != 0),
    CC_OPT_BOOL("mirror_views", e->mirror_views = v != 0),
    CC_OPT_BOOL("resident", e->resident_opt = v != 0),
    CC_OPT_INT("resident_idle_ms", 1, 10000, e->res_idle_ms = (int) v),
    CC_OPT_ACTION("prewarm_small_graphs", if (v) prewarm_small_calls(e)),
    CC_OPT_ACTION("forget_inclination_table", if (v) return forget_inclination_table(e)),
    // -- debugging
    CC_OPT_INT("timing_every", 1, INT32_MAX, e->timing_every = (int) v),
    CC_OPT_INT("check_input_lifetime", 0, 2, int rc = finish_batch(e); if (rc) return rc; e->check_input_lifetime = (int) v, e->live_inputs.clear()),
};

#undef CC_OPT_ACTION
#undef CC_OPT_TRI
#undef CC_OPT_INT
#undef CC_OPT_BOOL
#undef CC_OPT_APPLY

// the row of `name`, or nullptr (36 rows and a call that synchronises the engine first: a linear search)
inline const OptionDef* cc_option_find(const char* name)
{
    for (const OptionDef& d : CC_OPTIONS)
        if (strcmp(d.name, name) == 0)
            return &d;
    return nullptr;
}
