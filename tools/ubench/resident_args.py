#!/usr/bin/env python3
"""Driver of tools/ubench/resident_args.hip: the first link of a step launch under three argument shapes, plain build and
-mllvm -amdgpu-kernarg-preload-count build alternating, one process each.

    python tools/ubench/resident_args.py --build          # cross-compiles both programs (no GPU needed)
    python tools/ubench/resident_args.py [--runs 3]       # on the GPU; prints every run

Stops at the first program that does not end cleanly."""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "resident_args.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off"]
BUILDS = {"plain": [], "preload": ["-mllvm", "-amdgpu-kernarg-preload-count=16"]}   # 16: the toolchain caps it at the SGPRs it has left


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.build:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        for tag, extra in BUILDS.items():
            subprocess.check_call([hipcc] + FLAGS + extra + [SRC, "-o", os.path.join(HERE, "resident_args_" + tag)])
        return 0
    for run in range(a.runs):
        for tag in BUILDS:
            r = subprocess.run([os.path.join(HERE, "resident_args_" + tag), tag, "3"], timeout=120)
            if r.returncode != 0:
                print(f"resident_args_{tag} ended with status {r.returncode}: stopping", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
