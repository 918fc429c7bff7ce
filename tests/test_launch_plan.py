"""The launch plan (csrc/launch_plan.h), enumerated on the CPU.

Every form of every step kernel gives word-for-word identical results, so no output test can see a launch that went to the wrong
kernel: a handle that falls from its shape kernel to 8-lane groups passes every oracle tier and merely runs slower.  What decides
is one pure host function, `plan_launch`; this file compiles it ALONE with the host compiler (tests/sanitize/plan_host.cpp, ASan +
UBSan, run as a program of its own), feeds it a lattice of handles and calls, and holds every plan to the rules restated below in
words of this file's own -- nothing here imports the plan from the code under test.  Then the plans are held against the shipped
library: every lane-group plan names a kernel that is there, and every lane-group step, rollout and observation kernel that is
there is named by some plan.
"""
import itertools
import os
import subprocess
import sys
import tempfile

import pytest

from test_shape_kernels import REFERENCE, _kernel_stem, _match, _params, table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "marbler_amd", "csrc")
CLANG_DIRS = ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin")

PCP, WAREHOUSE, MT, SIMPLE, ARCTIC = range(5)                  # include/robogym.h RG_SCN_*
EXACT, CVXOPT = 0, 1                                           # RG_QP_*
NONE, LIDAR, POOL, DISTURB = range(4)                          # the side block that is on; also the kernel family it selects
STEP, ROLLOUT, OBS, STEP_RESIDENT, STEP_SHAPE = range(5)       # launch kinds (the last two: the plan's own answers to STEP)
DEFAULT, FORCE_GROUP, FORCE_TPE = range(3)                     # RG_STEP_KERNEL unset | group | tpe
FORM_BY_VALUE, FORM_RESIDENT, FORM_SHAPE = 1, 2, 16            # include/robogym.h RG_FORM_*
BATCHES = (1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385)
INT32_MAX = 2 ** 31 - 1
OUT = ("tpe", "family", "mode", "kind", "gw", "nt", "rollout", "gym", "rows", "resident", "shape", "envs_per_wave", "grid", "form",
       "image_wanted")


def admitted():
    """(scenario, n_agents, mode) that rg_create's check_params admits: 1..16 agents, ArcticTransport exactly 4, the interior-point
    mode at most 8."""
    for scn, mode in itertools.product(range(5), (EXACT, CVXOPT)):
        for n in range(1, 17):
            if (scn == ARCTIC and n != 4) or (mode == CVXOPT and n > 8):
                continue
            yield scn, n, mode


def min_envs_for_thread_per_env(scn, n, mode):
    """The measured cross-overs (profiles/r3_crossover_probe.txt, profiles/r5_ipm_crossover.jsonl), as a table of this file's."""
    if mode == CVXOPT:
        return 12288 if n == 5 else 20480
    return {2: 65536,
            3: 98304 if scn == PCP else 65536,
            4: {SIMPLE: 393216, ARCTIC: 131072}.get(scn, 196608),
            5: 49152 if scn == MT else 65536,
            6: {MT: 65536, WAREHOUSE: 262144, PCP: 98304}.get(scn, 131072)}.get(n, INT32_MAX)


@pytest.fixture(scope="module")
def driver():
    clang = next((os.path.join(d, "clang++") for d in CLANG_DIRS if os.path.exists(os.path.join(d, "clang++"))), None)
    assert clang, "ROCm's clang not found"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_host")
        subprocess.run([clang, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(HERE, "sanitize", "plan_host.cpp"), "-o", exe], check=True)

        def plans(cases):
            """cases: [dict] with the driver's input fields -> [dict] of the plan's."""
            keys = ("scn", "n", "mode", "E", "side", "force", "tpe_ok", "span", "resident", "shapes", "kind", "gym", "image", "image_shape")
            text = "".join(" ".join(str(int(c[k])) for k in keys) + "\n" for c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
            assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
            lines = r.stdout.splitlines()
            assert len(lines) == len(cases)
            return [dict(zip(OUT, map(int, ln.split()))) for ln in lines]

        yield plans


@pytest.fixture(scope="module")
def matched():
    """(scenario, n_agents) -> the reference shape its block matches (rg_shape_match, host code): the benchmark configurations."""
    ids = {}
    for scenario, ov in REFERENCE.items():
        p = _params(scenario, ov)
        ids[(int(p.scenario), int(p.n_agents))] = _match(p)
    assert sorted(ids.values()) == [r["id"] for r in table()]
    return ids


def lattice(matched):
    """Handles of the lane-group kernel (RG_STEP_KERNEL=group, as the GPU tiers run them) x calls."""
    cases = []
    for scn, n, mode in admitted():
        sid = matched.get((scn, n), 0) if mode == EXACT else 0
        images = [(0, 0), (1, 0)] + ([(1, sid)] if sid else [])
        for side, (kind, gym), span, resident, shapes, (image, image_shape), E in itertools.product(
                range(4), ((STEP, 0), (STEP, 1), (ROLLOUT, 0), (OBS, 0)), (0, 1), (0, 1), (0, 1), images, BATCHES):
            if side == POOL and scn == ARCTIC:   # refused by rg_set_teams
                continue
            cases.append(dict(scn=scn, n=n, mode=mode, E=E, side=side, force=FORCE_GROUP, tpe_ok=1, span=span, resident=resident,
                              shapes=shapes, kind=kind, gym=gym, image=image, image_shape=image_shape))
    return cases


@pytest.fixture(scope="module")
def planned(driver, matched):
    cases = lattice(matched)
    return cases, driver(cases)


def width(n):
    return 4 if n <= 4 else 8 if n <= 8 else 16


def slots(n, E):
    """Halve the env slots a wave uses while the batch still fits 1024 waves (one per SIMD)."""
    epw = 64 // width(n)
    while epw >= 2 and -(-E // (epw // 2)) <= 1024:
        epw //= 2
    return epw


def test_width_fill_and_grid(planned):
    """1. gw, envs_per_wave and grid; ArcticTransport runs full waves (envs_per_wave 0 = every slot)."""
    for c, pl in zip(*planned):
        assert not pl["tpe"] and pl["gw"] == width(c["n"]), (c, pl)
        epw = 64 // pl["gw"] if c["scn"] == ARCTIC else slots(c["n"], c["E"])
        assert pl["envs_per_wave"] == (0 if c["scn"] == ARCTIC else epw), (c, pl)
        assert pl["grid"] == -(-c["E"] // epw) and (pl["grid"] - 1) * epw < c["E"] <= pl["grid"] * epw, (c, pl)


def test_rows_resident_shape_and_form(planned, matched):
    """2. rows iff plain family, exact mode, single step without the gymma block, GW 8, span on, at most 4 envs per wave.
    3. resident implies rows and an image; a shape implies resident and is the one rg_shape_match gives the block.
    4. the form reported is the form taken.  8. image_wanted is `rows` of the handle's plain step."""
    seen = set()
    for c, pl in zip(*planned):
        rows = (c["side"] == NONE and c["mode"] == EXACT and c["kind"] == STEP and not c["gym"] and width(c["n"]) == 8 and
                bool(c["span"]) and c["scn"] != ARCTIC and slots(c["n"], c["E"]) <= 4)
        assert bool(pl["rows"]) == rows, (c, pl)
        resident = rows and bool(c["resident"]) and bool(c["image"])
        assert bool(pl["resident"]) == resident, (c, pl)
        shape = c["image_shape"] if resident and c["shapes"] else 0
        assert pl["shape"] == shape and shape in (0, matched.get((c["scn"], c["n"]))), (c, pl)
        assert pl["form"] == (FORM_SHAPE + shape if shape else FORM_RESIDENT if resident else FORM_BY_VALUE), (c, pl)
        assert pl["kind"] == (STEP_SHAPE if shape else STEP_RESIDENT if resident else c["kind"]), (c, pl)
        assert bool(pl["gym"]) == bool(c["gym"]) and bool(pl["rollout"]) == (c["kind"] == ROLLOUT), (c, pl)
        wanted = (c["side"] == NONE and c["mode"] == EXACT and width(c["n"]) == 8 and bool(c["span"]) and slots(c["n"], c["E"]) <= 4)
        assert bool(pl["image_wanted"]) == wanted, (c, pl)
        seen.add((bool(pl["rows"]), bool(pl["resident"]), bool(pl["shape"])))
    assert seen == {(False, False, False), (True, False, False), (True, True, False), (True, True, True)}


def test_family_mode_and_specialised_bodies(planned):
    """5. nt is the agent count only at GW 8, in the exact mode, for the step and rollout of the plain and team families without the
    gymma block; else 0.  6. a disturbed handle's observation launch is the plain family's; an observation runs the exact mode's
    kernel."""
    for c, pl in zip(*planned):
        family = NONE if (c["side"] == DISTURB and c["kind"] == OBS) else c["side"]
        mode = EXACT if c["kind"] == OBS else c["mode"]
        assert (pl["family"], pl["mode"]) == (family, mode), (c, pl)
        by_n = width(c["n"]) == 8 and mode == EXACT and c["kind"] in (STEP, ROLLOUT) and not c["gym"] and family in (NONE, POOL)
        assert pl["nt"] == (c["n"] if by_n else 0), (c, pl)


def test_kernel_choice(driver):
    """7. the thread-per-env kernel: a step or rollout of a handle without side block, where the kernel exists for the block, and
    RG_STEP_KERNEL=tpe asks for it or -- nothing forced -- the batch has reached the measured cross-over.  Any side block forces
    the lane-group kernel; with the block off again the choice is the default one (the plan is a function of the handle as it is)."""
    cases = []
    for scn, n, mode in admitted():
        thr = min_envs_for_thread_per_env(scn, n, mode)
        for E, side, kind, force, tpe_ok in itertools.product((1, 4096, thr - 1, thr), range(4), (STEP, ROLLOUT, OBS), range(3), (0, 1)):
            if side == POOL and scn == ARCTIC:
                continue
            cases.append(dict(scn=scn, n=n, mode=mode, E=E, side=side, force=force, tpe_ok=tpe_ok, span=1, resident=1, shapes=1,
                              kind=kind, gym=0, image=0, image_shape=0))
    chosen = 0
    for c, pl in zip(cases, driver(cases)):
        thr = min_envs_for_thread_per_env(c["scn"], c["n"], c["mode"])
        tpe = (c["kind"] != OBS and c["side"] == NONE and bool(c["tpe_ok"]) and
               (c["force"] == FORCE_TPE or (c["force"] == DEFAULT and c["E"] >= thr)))
        assert bool(pl["tpe"]) == tpe, (c, pl)
        assert pl["form"] == FORM_BY_VALUE and not pl["rows"] or not tpe, (c, pl)
        chosen += tpe
    assert chosen > 100


# ------------------------------------------------------------------ the plans against the shipped library
def kernel_stem(c, pl, shapes):
    """The mangled name (up to the end of its template arguments) of the kernel a lane-group plan names (csrc/step_group.h)."""
    scn, gw, nt, qpm = c["scn"], pl["gw"], pl["nt"], pl["mode"]
    obs, rollout, gym = int(pl["kind"] == OBS), pl["rollout"], pl["gym"]
    if pl["shape"]:
        return _kernel_stem(shapes[pl["shape"]])
    if pl["resident"]:
        return f"_ZN2rg11step_kernelILi{scn}ELi8ELb0ELi{nt}ELb0ELi16ELb1ETn"
    if pl["rows"]:
        return f"_ZN2rg11step_kernelILi{scn}ELi8ELb0ELi{nt}ELb0ELi16ETn"
    if pl["family"] == LIDAR:
        return f"_ZN2rg17lidar_step_kernelILi{scn}ELi{gw}ELb{obs}ELb{rollout}ELb{gym}ELi{qpm}EEEvNS_9LidarArgsE"
    if pl["family"] == POOL:
        return f"_ZN2rg16team_step_kernelILi{scn}ELi{gw}ELb{obs}ELi{nt}ELb{rollout}ELb{gym}ELi{qpm}EEEvNS_8TeamArgsE"
    if pl["family"] == DISTURB:
        return f"_ZN2rg19disturb_step_kernelILi{scn}ELi{gw}ELb{rollout}ELb{gym}ELi{qpm}EEEvNS_11DisturbArgsE"
    return f"_ZN2rg11step_kernelILi{scn}ELi{gw}ELb{obs}ELi{nt}ELb{rollout}ELb{gym}ELi{qpm}EEEvNS_10KernelArgsE"


# Kernels that are built but that no plan of the lattice reaches, with the reason.  (None today.)
UNREACHED = {}


def test_every_plan_names_a_shipped_kernel_and_every_kernel_is_named(planned):
    import isa_scan
    from marbler_amd import build as hip_build
    assert os.path.exists(hip_build.LIB), "librobogym_hip.so is not built"
    families = ("2rg11step_kernelI", "2rg17lidar_step_kernelI", "2rg16team_step_kernelI", "2rg19disturb_step_kernelI")
    with tempfile.TemporaryDirectory() as d:
        built = sorted(k for co in isa_scan.extract_code_objects(hip_build.LIB, d) for k in isa_scan.resources(co)
                       if any(f in k for f in families))
    assert len(built) > 300, len(built)
    shapes = {r["id"]: r for r in table()}
    stems = {kernel_stem(c, pl, shapes) for c, pl in zip(*planned)}
    named = set()
    for stem in sorted(stems):
        hits = [k for k in built if k.startswith(stem)]
        assert len(hits) == 1, f"a plan names {stem}: {len(hits)} such kernels in the library"
        named.add(hits[0])
    unreached = sorted(set(built) - named)
    assert unreached == sorted(UNREACHED), f"built but named by no plan: {[k for k in unreached if k not in UNREACHED][:10]}"
