"""The two device-side pieces a policy-in-the-loop kernel is built from, compiled (no GPU needed) into one multi-wave workgroup:

* the actor's tile computation (csrc/actor_body.inc) with the caller's own hooks for where a tile's rows lie and where their hidden
  state lives (here: LDS), run by both wavefronts of a hidden-64 tile;
* one gymma env step (step_group.h step_once) run by wavefront 0 alone, with WaveSync: every barrier of the step and of its fused
  reset sits under that wave's control flow, so none of them may be a workgroup barrier (the other wave would never meet it and
  the workgroup would hang).

The check is on the ISA: adding the step to the kernel adds no s_barrier.  Both kernels must also compile without scratch."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marbler_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROBE = r"""
#include "step_group.h"
#include "actor_common.h"

namespace rg {

template <bool WITH_STEP>
__global__ __launch_bounds__(128) void reuse_probe(const KernelArgs ka, const ActorArgs a, int row0) {
    {
        constexpr int H = 64, SPLIT = 2;
        __shared__ float hres[32 * H];   // the tile's hidden state, resident in LDS
#define RG_ACTOR_LOCATE(shared, E, set, base) base = row0
#define RG_ACTOR_HIDDEN_LOAD(r, k4) *reinterpret_cast<const float4 *>(&hres[(((r) - row0) & 31) * H + 4 * (k4)])
#define RG_ACTOR_HIDDEN_STORE(r, j, v) hres[(((r) - row0) & 31) * H + (j)] = (v)
#include "actor_body.inc"
#undef RG_ACTOR_LOCATE
#undef RG_ACTOR_HIDDEN_LOAD
#undef RG_ACTOR_HIDDEN_STORE
    }
    __syncthreads();
    if constexpr (WITH_STEP) {
        __shared__ Lds<4> lds;
        if (threadIdx.x < WAVE)
            step_once<RG_SCN_PREDATOR_CAPTURE_PREY, 4, false, 0, false, true, 0, void, WaveSync>(
                ka, lds, step_view(ka, 0, ka.p.n_agents, ka.p.obs_dim), static_cast<void *>(nullptr));
    }
    __syncthreads();
}

template __global__ void reuse_probe<false>(const KernelArgs, const ActorArgs, int);
template __global__ void reuse_probe<true>(const KernelArgs, const ActorArgs, int);

}  // namespace rg
"""


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def probe_isa():
    import isa_scan
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "probe.hip"), os.path.join(d, "probe.co")
        with open(src, "w") as f:
            f.write(PROBE)
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                        "--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj], check=True, capture_output=True)
        kernels = isa_scan.disassemble(obj)
        res = isa_scan.resources(obj)
    return kernels, res


def _kernel(kernels, with_step):
    name = [k for k in kernels if "reuse_probe" in k and re.search(r"ILb%dE" % int(with_step), k)]
    assert len(name) == 1, sorted(kernels)
    return name[0]


def test_wave_scope_step_adds_no_workgroup_barrier(probe_isa):
    kernels, _ = probe_isa
    count = {w: sum(1 for i in kernels[_kernel(kernels, w)] if i.op == "s_barrier") for w in (False, True)}
    assert count[False] > 0, "the actor's own barriers should be there"
    assert count[True] == count[False], f"step_once<WaveSync> put {count[True] - count[False]} workgroup barriers under wave 0's control flow"


def test_reuse_probe_has_no_scratch(probe_isa):
    kernels, res = probe_isa
    for w in (False, True):
        r = res[_kernel(kernels, w)]
        assert r["scratch"] == 0, r
