// extern "C" face of csrc/gangfit_label_plan.h for tests/test_label_plan_cpu.py (pure host code: g++ only, no HIP).
#include "gangfit_label_plan.h"

extern "C" void lp_plan(uint32_t n, const uint32_t* driver_rank, const uint32_t* exec_rank, int finalize_on_device, uint32_t out[7]) {
    const gfapi::LabelPlan p = gfapi::plan_labels(n, driver_rank, exec_rank, finalize_on_device != 0);
    out[0] = p.device_route;
    out[1] = p.driver_active;
    out[2] = p.exec_active;
    out[3] = (uint32_t)p.which;
    out[4] = p.max_rank;
    out[5] = p.width;
    out[6] = p.passes;
}
