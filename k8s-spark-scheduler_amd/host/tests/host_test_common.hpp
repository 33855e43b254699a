// host_test_common.hpp — what every test program of the host mirror shares: CHECK and its two counters, Mi / Gi, the context of
// the gpu half, a splitmix64 next() (for a program that defines HOST_TEST_SEED before including this) and the cpu / gpu / all
// dispatch of main.  Fixtures (Driver, NewNode, ...) differ per program and stay there.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>

#include "extender.hpp"

using namespace gangfit::host;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checked;                                                           \
        if (!(cond)) {                                                         \
            ++g_failed;                                                        \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);        \
        }                                                                      \
    } while (0)

static const int64_t Mi = 1024 * 1024, Gi = 1024 * Mi;
static gf_ctx* g_ctx = nullptr;  // the gpu half's context; stays NULL in the cpu half

#ifdef HOST_TEST_SEED
static uint64_t g_rng = HOST_TEST_SEED;
static inline uint64_t next() {
    g_rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
#endif

// main: `cpu` (the default) runs the half that needs no GPU, `gpu` the half that drives the device through the C ABI on g_ctx,
// `all` both.  Exit code 0 = all passed, 1 = a CHECK failed, 2 = no device.
static inline int RunHostTests(int argc, char** argv, void (*cpu_half)(), void (*gpu_half)()) {
    (void)setenv("GPU_MAX_HW_QUEUES", "16", 0);  // the deployment's part ("Deployment")
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "cpu" || mode == "all") cpu_half();
    if (mode == "gpu" || mode == "all") {
        if (gf_init(nullptr, 0, &g_ctx) != GF_OK) {
            std::printf("FAIL gf_init: no gfx950 device (there is no CPU fallback)\n");
            return 2;
        }
        gpu_half();
        gf_destroy(g_ctx);
    }
    std::printf("%s: %d checks, %d failed\n", mode.c_str(), g_checked, g_failed);
    return g_failed == 0 ? 0 : 1;
}
