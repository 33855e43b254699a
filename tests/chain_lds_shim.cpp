// chain_lds_shim.cpp — what tests/test_chain_lds_layout_cpu.py loads through ctypes: the two layout functions of
// gangfit_chain_lds.h with every offset copied out in field order (`bytes` last), and the record sizes and capacities the layouts
// depend on.  Host code only (g++ -std=c++17 -I include -I k8s-spark-scheduler_amd/csrc).  With -DCHAIN_LDS_MAIN it is a stand-alone
// program that walks the test's grid once (for a run under -fsanitize=address,undefined).
#include <cstdio>

#include "gangfit_chain_lds.h"

using namespace gangfit;
using namespace gangfit::chain_lds;

extern "C" {

// kAppStage, kZStage, kMaxShapes, kZRunMax, then the sizes of ZonedShared, Exchange, FifoShared, NApp, gf_app
void cl_constants(uint64_t* out) {
    const uint64_t v[9] = {(uint64_t)kAppStage, (uint64_t)kZStage, kMaxShapes, kZRunMax, sizeof(ZonedShared), sizeof(Exchange),
                           kFifoSharedBytes, kNAppBytes, sizeof(gf_app)};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}

int cl_wide(uint32_t lds_slots, uint32_t n_chunks, uint64_t* out) {
    const WideChainLds L = wide_chain_lds(lds_slots, n_chunks);
    const size_t v[] = {L.lcpu, L.lmem, L.lgpu, L.lmax, L.lxm, L.exchange, L.shared, L.dirty, L.reserve, L.bytes};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}

int cl_zoned(uint32_t lds_slots, uint32_t n_chunks, uint32_t n_views, uint32_t n_waves, uint32_t n_shapes, uint64_t* out) {
    const ZonedLds L = zoned_lds(lds_slots, n_chunks, n_views, n_waves, n_shapes);
    const size_t v[] = {L.stage, L.nstage, L.shared, L.lmasks, L.lcm, L.lruns, L.sbx, L.sbd, L.ltab, L.spare_words, L.reserve, L.bytes};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

#ifdef CHAIN_LDS_MAIN
int main() {
    const uint32_t chunks[] = {1, 2, 63, 64, 65, 157, 782, 1563}, waves[] = {4, 8, 16}, shapes[] = {0, 4, 8, 16, 32, 64};
    uint64_t out[32], sum = 0, n = 0;
    cl_constants(out);
    for (uint32_t nc : chunks) {
        const uint32_t slots[] = {0, 64, 128, 64 * nc, 1, 63, 64 * nc - 1};
        for (uint32_t ls : slots) {
            sum += out[cl_wide(ls, nc, out) - 1], ++n;
            if (ls % 64u != 0u) continue;
            for (uint32_t nv = 1; nv <= 17; ++nv)
                for (uint32_t ns : shapes)
                    for (uint32_t nw : waves) sum += out[cl_zoned(ls, nc, nv, nw, ns, out) - 1], ++n;
        }
    }
    std::printf("%llu layouts, %llu bytes in all\n", (unsigned long long)n, (unsigned long long)sum);
    return 0;
}
#endif
