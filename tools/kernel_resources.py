"""Registers, spills, scratch and LDS of every hot:: kernel of a built library, from its gfx950 code objects (no GPU needed).

  python tools/kernel_resources.py [--lib hot_amd/csrc/libhotmi355x.so] [--out profiles/kernel_resources.txt]

Columns: the workgroup size the kernel is compiled for (its __launch_bounds__), VGPRs (+ AGPRs), SGPRs, spilled VGPRs (to scratch memory),
spilled SGPRs (to lanes of a vector register: no memory traffic), scratch bytes per lane, static LDS bytes (dynamic LDS is the launch's),
and the wavefronts per SIMD the register file allows (512 registers per lane, granules of 8, at most 8).  tests/test_kernel_resources.py
holds the rule the table is checked against."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hot_amd  # noqa: E402
from hot_amd import kernel_resources as kr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=hot_amd.LIB_PATH)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [k for k in kr.read(args.lib) if k["name"].startswith("hot::")]
    lines = [f"kernel resources of {os.path.relpath(args.lib, ROOT)}, gfx950: {len(ks)} hot:: kernels, "
             f"{sum(1 for k in ks if k['scratch'])} with scratch memory, {sum(1 for k in ks if k['vgpr_spill'])} with spilled VGPRs",
             f"{'kernel':64s} {'wg<=':>5s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'LDS':>7s} {'waves/SIMD':>10s}"]
    for k in ks:
        lines.append(f"{k['name'][5:]:64s} {k['max_threads']:5d} {k['vgpr']:5d} {k['agpr']:5d} {k['sgpr']:5d} {k['vgpr_spill']:6d} {k['sgpr_spill']:6d} "
                     f"{k['scratch']:7d} {k['lds']:7d} {k['waves_per_simd']:10d}")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
