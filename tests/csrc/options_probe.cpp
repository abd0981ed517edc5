// Host-only probe of continuous_clustering_amd/csrc/cc_options.h for tests/test_options_cpu.py: the option table without the engine.
// Prints one line per row ("row <name> <kind> <lo> <hi>"), then answers "<name> <value>" lines from standard input with
// "clamp <name> <value> <clamped>" or "unknown <name>". No HIP, no GPU.
#include <cinttypes>
#include <cstdio>

// what cc_engine.hip has in scope where it includes the header: the engine type (only named here) and the two bounds that are constants of
// kernel headers (their default values: cc_device.h, cc_k_scan.h)
#define CC_OPTIONS_TABLE_ONLY
struct cc_engine;
constexpr int TREE_SLOTS = 256;
namespace cck
{
constexpr int SL_CAP = 8192;
}
#include "../../continuous_clustering_amd/csrc/cc_options.h"

int main()
{
    static const char* const kinds[] = {"bool", "int", "tri", "action"};
    for (const OptionDef& d : CC_OPTIONS)
        printf("row %s %s %" PRId64 " %" PRId64 "\n", d.name, kinds[d.kind], d.lo, d.hi);
    char name[128];
    int64_t value = 0;
    while (scanf("%127s %" SCNd64, name, &value) == 2)
    {
        const OptionDef* d = cc_option_find(name);
        if (d)
            printf("clamp %s %" PRId64 " %" PRId64 "\n", name, value, cc_option_clamp(*d, value));
        else
            printf("unknown %s\n", name);
    }
    return 0;
}
