// Stand-alone driver of csrc/gangfit_label_plan.h over the cases of tests/test_label_plan_cpu.py, for a build with
// -fsanitize=address,undefined: every array is an exact-size heap allocation, so a read past either end is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gangfit_label_plan.h"

using gfapi::kLabelUnranked;
using gfapi::LabelPlan;

static int failures = 0;

static const uint32_t* heap(const std::vector<uint32_t>& v, std::vector<uint32_t*>* owned) {
    uint32_t* p = (uint32_t*)std::malloc(v.size() * sizeof(uint32_t) + (v.empty() ? 1 : 0));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(uint32_t));
    owned->push_back(p);
    return p;
}

static void expect(const char* name, const LabelPlan& p, bool device, bool da, bool xa, int which, uint32_t max_rank, uint32_t width,
                   uint32_t passes) {
    const bool ok = p.device_route == device && p.driver_active == da && p.exec_active == xa && p.which == which &&
                    p.max_rank == max_rank && p.width == width && p.passes == passes;
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: device %d active %d %d which %d max %u width %u passes %u\n", name, p.device_route, p.driver_active,
                    p.exec_active, p.which, p.max_rank, p.width, p.passes);
    }
}

int main() {
    const uint32_t U = kLabelUnranked;
    std::vector<uint32_t*> owned;
    auto P = [&](const std::vector<uint32_t>& d, bool has_d, const std::vector<uint32_t>& x, bool has_x, bool dev) {
        const uint32_t n = (uint32_t)(has_d ? d.size() : x.size());
        return gfapi::plan_labels(n, has_d ? heap(d, &owned) : nullptr, has_x ? heap(x, &owned) : nullptr, dev);
    };
    expect("no arrays", P({}, false, {}, false, true), true, false, false, 0, 0, 0, 0);
    expect("empty arrays", P({}, true, {}, true, true), true, false, false, 0, 0, 0, 0);
    expect("all unranked", P({U, U, U}, true, {U, U, U}, true, true), true, false, false, 0, 0, 0, 0);
    expect("all equal", P({7, 7, 7, 7}, true, {}, false, true), true, false, false, 0, 0, 0, 0);
    expect("one node", P({3}, true, {U}, true, true), true, false, false, 0, 0, 0, 0);
    expect("max 0", P({0, U}, true, {}, false, true), true, true, false, 1, 0, 1, 1);
    expect("max 254", P({254, 0, U}, true, {}, false, true), true, true, false, 1, 254, 8, 1);
    expect("max 255", P({0, 255}, true, {}, false, true), true, true, false, 1, 255, 9, 2);
    expect("max 256", P({256, U, 1}, true, {}, false, true), true, true, false, 1, 256, 9, 2);
    expect("max 2^16-1", P({65535, 1}, true, {}, false, true), true, true, false, 1, 65535, 17, 3);
    expect("max 2^32-2", P({U - 1, 0, U}, true, {}, false, true), true, true, false, 1, U - 1, 32, 4);
    expect("driver is L", P({0, 1, U}, true, {5, 9, 5}, true, true), true, true, true, 1, 1, 2, 1);
    expect("exec is L: no driver array", P({}, false, {5, 9, 5}, true, true), true, false, true, 2, 9, 4, 1);
    expect("exec is L: driver array re-sorts nothing", P({4, 4, 4}, true, {5, 9, U}, true, true), true, false, true, 2, 9, 4, 1);
    expect("host option", P({0, 1, U}, true, {5, 9, 5}, true, false), false, true, true, 1, 1, 2, 1);
    {  // a larger array: the scan reads exactly n entries
        std::vector<uint32_t> big(100000);
        for (size_t i = 0; i < big.size(); ++i) big[i] = (uint32_t)(i % 300);
        big[777] = U;
        expect("100000 nodes", P(big, true, big, true, true), true, true, true, 1, 299, 9, 2);
    }
    for (uint32_t* p : owned) std::free(p);
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "label plan ok", failures);
    return failures ? 1 : 0;
}
