// td_targets_absent.cpp -- the entry points of csrc/robogym_td_targets.hip for the sanitized host library
// (marbler_amd/build.py build_host_sanitized), which does NOT hold that translation unit: its host half runs under ASan + UBSan in
// a stand-alone program of its own (td_targets_host.cpp).  The library only has to export every function include/robogym.h
// declares (tests/test_host.py) with the struct sizes the binding checks on load; a call is refused.
#include "../../include/robogym.h"

extern "C" int rg_sizeof_mixer_weights(void) { return static_cast<int>(sizeof(rg_mixer_weights)); }
extern "C" int rg_sizeof_td_targets_io(void) { return static_cast<int>(sizeof(rg_td_targets_io)); }
extern "C" const char *rg_td_targets_last_error(void) { return "rg_td_targets: not part of the sanitized host library"; }
extern "C" int rg_td_targets(const rg_mixer_weights *, const rg_td_targets_io *, void *) { return -100; }
