// TEST BUILD ONLY (tests/test_sanitizers.py), next to launch_stubs.cpp: the sampled actor launch lives in the device translation
// unit csrc/actor_mfma.hip, which the host-only sanitizer build does not contain.  The policy rollout's sampled launchers need no
// stub: csrc/robogym_capi.hip declares them weak and refuses to run without them.
#include "kernel_args.h"

extern "C" int rg_actor_forward_sample(const rg_actor_weights *, int32_t, int32_t, const float *, int32_t, int32_t, const uint8_t *,
                                       float *, float *, int32_t *, const float *, float *, void *) { return -100; }
