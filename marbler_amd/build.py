"""Build librobogym_hip.so (HIP kernels + C ABI) in-tree for gfx950.

    python -m marbler_amd.build

hipcc cross-compiles without a GPU.  -ffp-contract=off: the kernels' float arithmetic is an
explicit sequence of IEEE operations (csrc/sim_math.h) that the CPU oracle reproduces bit for
bit; implicit fma contraction would break that.
"""
import glob
import os
import re
import shlex
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librobogym_hip.so")
# The files that are a translation unit each.  The lane-group step kernels' units and the policy rollouts' are derived below
# (group_units, policy_units), each from one generic source.
SOURCES = ["robogym_kernels.hip", "robogym_resident.hip", "robogym_resident_shapes.hip", "robogym_tpe.hip", "robogym_rollout_tpe.hip",
           "robogym_capi.hip", "actor_mfma.hip", "robogym_team.hip", "robogym_render.hip", "robogym_episodes.hip",
           "robogym_actor_unroll.hip", "robogym_td_targets.hip", "robogym_nstep_returns.hip", "robogym_gru_scan.hip",
           "robogym_mixer_grad.hip"]
GROUP_UNIT, POLICY_UNIT = "robogym_group_unit.hip", "robogym_policy_unit.hip"
# every header of csrc/ (a forgotten one would mean a stale library), and the C ABI's
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(CSRC, "probes", "*.h"))) + \
          [os.path.join(HERE, "..", "include", h) for h in ("robogym.h", "robogym_returns.h", "robogym_learn.h")]
ARCH = "gfx950"
# Per-file flags (results are bit-identical either way: the same IEEE operations; tools/ab_job.sh measured them).
# * thread-per-env kernels: WITHOUT the SLP vectoriser.  Left on, it pairs the x / y halves of the float arithmetic into
#   v_pk_{add,mul,fma}_f32, which need even-aligned register pairs (more spills at N = 6, a kernel already compiled onto a
#   register budget): N = 6 272 -> 213 us (-22 %) at 524 288 envs, MaterialTransport N = 6 473 -> 386, N = 5 158.5 -> 152.1, N = 4 99 -> 94.
#   What a packed instruction is worth by itself was measured in round 5 (tools/ubench/issue.py, profiles/r5_issue_ubench.txt:
#   independent streams, flop / clk / SIMD): at this kernel's TWO waves per SIMD v_pk_fma_f32 issues 1.43 x the work of two
#   v_fma_f32 (55.8 against 38.9) but v_pk_mul + v_pk_add only 1.06 x the unfused pair (28.2 against 26.5) -- and the step
#   is unfused arithmetic for the most part (-ffp-contract=off; fma only where the float spec says so): the 6-43 % on the
#   instructions that could be paired does not pay for the registers the pairing costs here.  (At ONE wave per SIMD -- the
#   lane-group kernel's regime -- the same instructions are worth 1.86-2.0 x: hence the opposite flag below.)
# * lane-group kernels: the opposite, -mllvm -slp-threshold=-60 (pack wherever possible; 1 083 -> 1 227 packed f32 instructions
#   per translation unit): one wave per SIMD issues an instruction every ~5.5 cycles whatever its width (packed / scalar = 2.02
#   for fma, 1.86 for mul + add in the round-5 microbenchmark), so every pair packed is an issue slot saved -- headline launch
#   13.16 -> 12.73 us, Warehouse 4096 x 8 12.59 -> 12.40, rg_rollout 8.23 -> 7.97 us per step.
# Round 3 found that ONE thread-per-env instantiation (MaterialTransport, N = 7) computes wrong poses under
# -O3 -fno-slp-vectorize.  Round 4 found why (tools/n7_bisect/): ROCm 7.2's register allocator placed
# VGPR -> AGPR live-range split copies at the top of an `if`'s join block BEFORE the `s_or_b64 exec` that restores the exec
# mask -- an SGPR copy of the earlier SGPR allocation sat in front of it and ended what LLVM takes for the block prologue --
# so the saves ran for the `then` lanes only.  A compiler defect, not a property of this source (the same source is clean
# under ASan / UBSan / MSan on the host, tests/test_sanitizers.py); whether a build has it is visible in the ISA, and
# tests/test_kernel_resources.py scans every kernel of the shipped library for it (tools/isa_scan.py exec_prologue).
# The N = 7, 8 instantiations were never dispatched and are no longer built.
GROUP_SLP = ["-mllvm", "-slp-threshold=-60"]
# The interior-point mode's lane-group kernels (their own translation units) are long chains of binary64 arithmetic with
# independent strands beside them: the max-ILP scheduling strategy interleaves the strands (round 5, whole-library A/B on one box:
# interior-point mode 4096 x 5 141.8 -> 134.3 us, Warehouse 4096 x 8 607 -> 548, MaterialTransport 2048 x 6 unchanged; exact mode
# 12.70 -> 12.74, 32 768 envs 27.1 -> 29.0: NOT for the other files).  The one-lane-per-env interior-point kernels stay with the
# default strategy: under max-ILP the N = 5 one shows the exec-prologue shape isa_scan looks for.
IPM_SCHED = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# The resident form of the row kernels (robogym_resident.hip; kernel_args.h ResidentCall): its leading kernel arguments -- the
# image's address, the actions, the seed, auto_reset, the grid: 8 dwords; the hidden grid size lies behind the by-value rg_step_io
# and would not be among them -- are handed to a wave in scalar registers by the command processor instead of being fetched from the argument
# segment, which a host launch has just written.  The flag asks for up to 16 dwords and the compiler takes what precedes the
# first by-value struct; it changes every kernel of a translation unit it is given to, hence a file of its own.
# tools/ubench/resident_args.py priced it (profiles/resident_args_ubench.txt).
RESIDENT_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
# The unroll kernels (actor_unroll.h) run actor_body.inc inside a time loop, and inside a loop the block placement duplicates the
# join block of the arg-max pass's `if (c < A)`: the taken path falls into its own copy of `s_or_b64 exec`, the skipped path
# branches to another.  Correct code -- the compare in front of that copy belongs to the `then` lanes -- but it is the shape
# tools/isa_scan.py exec_prologue reports (vector instructions between a label, here the inner `if (ok && a.q)`'s join, and an
# exec restore), and tests/test_kernel_resources.py scans every shipped kernel.  Without the duplication the kernels have the
# layout actor_kernel has, the same registers and LDS, and the scan is clean.
UNROLL_LAYOUT = ["-mllvm", "-tail-dup-placement=false"]


def group_flags(mode):
    """The flags of a translation unit of lane-group kernels, whatever its family -- plain, lidar (step_group.h
    lidar_step_kernel), team (team_step_kernel), pose disturbance (disturb_step_kernel) -- and the policy rollouts': GROUP_SLP,
    and IPM_SCHED on top in the interior-point mode.  Hence a mode's kernels never share a unit with the other mode's: the
    exact-projection kernels are better off with the default scheduling strategy (the figures above)."""
    return GROUP_SLP + (IPM_SCHED if mode == "RG_QP_CVXOPT" else [])


FILE_FLAGS = {"robogym_tpe.hip": ["-fno-slp-vectorize"], "robogym_rollout_tpe.hip": ["-fno-slp-vectorize"],
              # the plain and the team family's single launches of the exact mode, next to the reset kernel and the index writer
              "robogym_kernels.hip": group_flags("RG_QP_EXACT"), "robogym_team.hip": group_flags("RG_QP_EXACT"),
              "robogym_resident.hip": GROUP_SLP + RESIDENT_PRELOAD,
              # the reference shapes' resident kernels (kernel_args.h RG_REF_SHAPES): the same kernels, the same flags
              "robogym_resident_shapes.hip": GROUP_SLP + RESIDENT_PRELOAD,
              "robogym_actor_unroll.hip": UNROLL_LAYOUT}
# the rows of RG_GROUP_ENTRIES that a file above defines itself, next to a kernel or a launcher of its own
OWN_ENTRIES = {"launch_step", "launch_obs", "launch_team_step", "launch_team_obs", "launch_step_resident", "launch_step_shape"}


def group_rows():
    """The rows of csrc/kernel_args.h RG_GROUP_ENTRIES -- the one list of the lane-group entries -- as (entry, family, mode, kind)."""
    with open(os.path.join(CSRC, "kernel_args.h")) as f:
        table = re.search(r"#define RG_GROUP_ENTRIES\(X\)((?:.*\\\n)*.*)", f.read()).group(1)
    return re.findall(r"X\((\w+), (\w+), (\w+), (\w+)\)", table)


def group_units():
    """The lane-group units compiled from GROUP_UNIT, as (object name, source, flags, defines).  A unit is a family's single
    launches of one solver mode (step, and obs where the family has one) or its rollout, and is handed its rows as they stand."""
    units = {}
    for entry, family, mode, kind in group_rows():
        if entry not in OWN_ENTRIES:
            units.setdefault((family, mode, kind == "GROUP_ROLLOUT"), []).append(f"X({entry},{family},{mode},{kind})")
    # (the object's name: robogym_lidar_cvxopt_rollout for GROUP_LIDAR, RG_QP_CVXOPT, rollout)
    return [(f"robogym_{family[6:]}_{mode[6:]}{'_rollout' if rollout else ''}".lower(), GROUP_UNIT, group_flags(mode),
             ["RG_UNIT_ROWS=" + "".join(rows)]) for (family, mode, rollout), rows in units.items()]


def policy_units():
    """rg_policy_rollout's units: POLICY_UNIT per (hidden size, sampling), lane-group kernels of the exact mode."""
    return [(f"robogym_policy{'_sample' if sample else ''}_h{h}", POLICY_UNIT, group_flags("RG_QP_EXACT"),
             [f"RG_UNIT_H={h}", f"RG_UNIT_SAMPLE={sample}"]) for sample in (0, 1) for h in (64, 128)]


def units():
    """Every translation unit of the library: (object name, source, per-unit flags, the unit's own defines)."""
    return [(os.path.splitext(s)[0], s, FILE_FLAGS.get(s, []), []) for s in SOURCES] + group_units() + policy_units()


BASE_FLAGS = [f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
STAMP = LIB + ".flags"


def hipcc_path():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (ROCm 7.x expected under /opt/rocm)")


def flags_stamp(defines=(), extra=(), file_flags=True):
    """What a library was built with, as one string: the rebuild check compares it (a library left behind by an A/B build
    with other flags is stale, whatever its mtime)."""
    return repr((BASE_FLAGS, sorted(defines), list(extra), [(n, s, f if file_flags else [], d) for n, s, f, d in units()]))


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + [GROUP_UNIT, POLICY_UNIT]] + HEADERS + [os.path.abspath(__file__)]
    if any(os.path.getmtime(d) > t for d in deps):
        return True
    try:
        with open(STAMP) as f:
            return f.read() != flags_stamp()
    except OSError:
        return True


def build(force=False, verbose=False, defines=(), out=None):
    """defines / out: diagnostic variants (e.g. defines=("RG_STAMPS",), out=".../librobogym_stamps.so").  The environment
    variables RG_EXTRA_HIPCC_FLAGS / RG_NO_FILE_FLAGS (A/B builds, tools/ab_job.sh) apply to such variants only: the shipped
    library is always built with the flags above."""
    extra = os.environ.get("RG_EXTRA_HIPCC_FLAGS", "").split()
    no_file_flags = bool(os.environ.get("RG_NO_FILE_FLAGS"))
    if out is None:
        if not force and not needs_build():
            return LIB
        if extra or no_file_flags:
            # a shell that still exports an A/B flag must not change (or block) the shipped build: its flags are fixed above
            import warnings
            warnings.warn("RG_EXTRA_HIPCC_FLAGS / RG_NO_FILE_FLAGS are for diagnostic variants (build(out=...)) and are IGNORED for the "
                          "shipped library, whose flags are fixed in marbler_amd/build.py")
            extra, no_file_flags = [], False
    shipped = out is None
    out = out or LIB
    # one object per translation unit, compiled side by side (the kernel instantiations dominate:
    # ~2 min each for the lane-group files, ~1 min for the thread-per-env ones), then one link
    objdir = os.path.join(HERE, "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    flags = BASE_FLAGS + [f"-D{d}" for d in defines] + extra
    objs, procs = [], []
    for name, src, unit_flags, unit_defines in units():
        obj = os.path.join(objdir, name + ".o")
        per_file = [] if no_file_flags else unit_flags   # (A/B builds)
        cmd = [hipcc_path()] + flags + per_file + [f"-D{d}" for d in unit_defines] + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(shlex.join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    link = [hipcc_path(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    with open(out + ".flags", "w") as f:
        f.write(flags_stamp(defines, extra, not no_file_flags) if not shipped else flags_stamp())
    return out


def build_host_sanitized(out=None):
    """CPU sanitizer tier: the C ABI's host half (csrc/robogym_capi.hip) compiled for the HOST ONLY with
    ASan + UBSan, linked against tests/sanitize/launch_stubs.cpp in place of the device translation units; with it the host half
    of csrc/robogym_render.hip (rg_render's argument checks: handle-free, it needs no stub) and of csrc/robogym_episodes.hip
    (rg_episodes_append's, likewise) and of csrc/robogym_actor_unroll.hip (rg_actor_unroll's, likewise).  csrc/robogym_td_targets.hip
    is NOT part of it -- its host half runs under the sanitizers in a stand-alone program (tests/test_td_targets_host_sanitized.py);
    tests/sanitize/td_targets_absent.cpp only exports its entry points, so that the library declares what the header declares.
    Used by tests/test_sanitizers.py for the no-GPU cases of tests/test_host.py; never shipped.  (GPU ASan is
    not available on this pool: sanitizers run on the CPU build only.)"""
    out = out or os.path.join(HERE, "build", "librobogym_capi_asan.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    stubs = os.path.join(HERE, "..", "tests", "sanitize", "launch_stubs.cpp")
    stubs_sample = os.path.join(HERE, "..", "tests", "sanitize", "launch_stubs_sample.cpp")   # rg_actor_forward_sample
    cmd = [hipcc_path(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fPIC", "-shared", "-std=c++17", "-DRG_RENDER_HOST_ONLY",
           "-DRG_EPISODES_HOST_ONLY", "-DRG_UNROLL_HOST_ONLY", "-I", CSRC, os.path.join(CSRC, "robogym_capi.hip"),
           os.path.join(CSRC, "robogym_render.hip"), os.path.join(CSRC, "robogym_episodes.hip"),
           os.path.join(CSRC, "robogym_actor_unroll.hip"), stubs, stubs_sample,
           os.path.join(HERE, "..", "tests", "sanitize", "td_targets_absent.cpp"), "-o", out]
    subprocess.check_call(cmd)
    return out


def asan_runtime():
    """clang's shared ASan runtime (to LD_PRELOAD into the python process that loads the sanitized library)."""
    return subprocess.check_output([hipcc_path(), "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
