// Host-side check of q1_step_plan (lac_amd/csrc/lac_select.h) -- test infrastructure.
//
// C wrappers for ctypes (tests/test_step_select_host.py).  Plain C++: nothing else is linked.
#include <stdint.h>

#include "lac_select.h"

extern "C" {

// o[4]: fused, rc, threads, R
void ssc_step_plan(int cus, int64_t V, int type_bytes, int64_t streams, int mode, int64_t *o) {
    const Q1StepPlan p = q1_step_plan(cus, V, type_bytes, streams, mode);
    o[0] = p.fused, o[1] = p.rc, o[2] = p.threads, o[3] = p.R;
}

// o[4]: kQ1StepMaxVec, kQ1StepMaxStreams, kQ1StepMaxThreads, kQ1StepMaxR
void ssc_consts(int64_t *o) {
    o[0] = kQ1StepMaxVec, o[1] = kQ1StepMaxStreams, o[2] = kQ1StepMaxThreads, o[3] = kQ1StepMaxR;
}

}  // extern "C"
