"""The host half of rg_mixer_forward / rg_mixer_backward (csrc/robogym_mixer_grad.hip with -DRG_MIXER_GRAD_HOST_ONLY) under
ASan + UBSan, in a stand-alone program with its own main and launch stub (tests/sanitize/mixer_host.cpp): compiled for the host
alone, run as a child process.  Nothing is loaded into this interpreter and no device is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "marbler_amd", "csrc", "robogym_mixer_grad.hip"), os.path.join(ROOT, "tests", "sanitize", "mixer_host.cpp")]
OUT = os.path.join(ROOT, "marbler_amd", "build", "host_sim")


def build_program():
    from marbler_amd import build as hip_build
    try:
        hipcc = hip_build.hipcc_path()
    except RuntimeError as exc:
        pytest.skip(str(exc))
    exe = os.path.join(OUT, "mixer_host_asan")
    deps = SRC + [os.path.join(ROOT, "include", "robogym.h"), os.path.join(ROOT, "include", "robogym_learn.h"),
                  os.path.join(ROOT, "marbler_amd", "csrc", "host_checks.h"), os.path.abspath(__file__)]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    os.makedirs(OUT, exist_ok=True)
    # (the sanitizers are for the host compilation alone: the option is handed to the host side, and no device code is built)
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-std=c++17", "-Wall", "-DRG_MIXER_GRAD_HOST_ONLY"] + SRC + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def test_host_half_of_the_mixer_entries_is_clean_under_asan_ubsan():
    exe = build_program()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1:detect_stack_use_after_return=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("mixer_host: ") and " 0 failed" in last and " 24 launches reached the stub" in last, last
    assert int(last.split()[1]) >= 300, last
