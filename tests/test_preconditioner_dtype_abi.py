"""CPU-side checks of the mixed-precision switch (include/hot_mi355x.h hot_set_preconditioner_dtype): the two entry points are
declared, exported and bound, hot_config and the ABI version did not move, and the new kernels came out of the compiler without scratch while
no existing kernel's registers, LDS or scratch changed."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hot_amd
from hot_amd import binding, kernel_resources as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hot_set_preconditioner_dtype", "hot_get_preconditioner_dtype")
NEW_KERNELS = ("k_mg32_matrix<false>", "k_mg32_matrix<true>", "k_mg32_absmax", "k_mg32_enter", "k_mg32_exit", "k_mg32_convert<double, float>",
               "k_mg32_convert<float, double>")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "hot_mi355x.h"
int main(void)
{
    int (*set)(hot_ctx*, int32_t) = hot_set_preconditioner_dtype;
    int (*get)(hot_ctx*, int32_t*) = hot_get_preconditioner_dtype;
    printf("%zu %zu %zu %d %d\n", offsetof(hot_config, deterministic), offsetof(hot_config, reserved), sizeof(hot_config), HOT_ABI_VERSION, set != 0 && get != 0);
    return 0;
}
"""


def _lib():
    if not os.path.exists(hot_amd.LIB_PATH):
        hot_amd.build()
    return hot_amd.load()


def test_header_declares_the_switch():
    hdr = open(os.path.join(ROOT, "include", "hot_mi355x.h")).read()
    assert re.search(r"\bint\s+hot_set_preconditioner_dtype\s*\(\s*hot_ctx\s*\*\s*,\s*int32_t\s+dtype\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+hot_get_preconditioner_dtype\s*\(\s*hot_ctx\s*\*\s*,\s*int32_t\s*\*\s*dtype\s*\)\s*;", hdr)
    assert re.search(r"#define HOT_ABI_VERSION 7\b", hdr)
    for name in NAMES:  # HIP product only: the CPU checker is loaded through the same binding and does not export them
        assert name[4:] in hot_amd.PRODUCT_ONLY_SYMBOLS and name[4:] not in hot_amd.ABI_SYMBOLS
    # the binding's lists and the header name the same entry points (what tests/test_abi_load.py::test_header_symbols_exported checks)
    declared = set(re.findall(r"\b(hot_[a-z0-9_]+)\s*\(", hdr)) - {"hot_ctx"}
    assert {"hot_" + s for s in hot_amd.ABI_SYMBOLS + hot_amd.PRODUCT_ONLY_SYMBOLS} == declared
    adapter = open(os.path.join(ROOT, "include", "hot_adapter.hpp")).read()
    assert "hot_set_preconditioner_dtype(ctx" in adapter and "hot_get_preconditioner_dtype(ctx" in adapter


def test_library_exports_the_switch():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib.lib, name), name
    assert lib.fn["abi_version"]() == 7 == binding.ABI_VERSION
    assert callable(hot_amd.Context.set_preconditioner_dtype)
    assert isinstance(hot_amd.Context.preconditioner_dtype, property)
    # not a hot_config field: the keyword is the binding's
    assert not hasattr(binding.hot_config, "preconditioner_dtype")
    with pytest.raises(KeyError):
        lib.default_config(preconditioner_dtype=0)


def test_header_layout_did_not_move(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    libdir = os.path.dirname(_lib().path)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lhotmi355x", "-Wl,-rpath," + libdir, "-o", str(exe)])
    off_det, off_res, size, abi, linked = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert off_det == binding.hot_config.deterministic.offset
    assert off_res == binding.hot_config.reserved.offset == off_det + 4
    assert size == C.sizeof(binding.hot_config)
    assert abi == binding.ABI_VERSION == 7
    assert linked == 1


def _table(text):
    """kernel name -> (VGPR, AGPR, vspill, scratch, LDS) of a profiles/kernel_resources.txt"""
    out = {}
    for line in text.splitlines()[2:]:
        m = re.match(r"^(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        assert m, line
        wg, vgpr, agpr, sgpr, vspill, sspill, scratch, lds, waves = (int(v) for v in m.groups()[1:])
        out[m.group(1)] = (vgpr, agpr, vspill, scratch, lds)
    return out


def test_new_kernels_have_no_scratch_and_no_existing_kernel_moved():
    lib = _lib()
    missing = kr.tools_missing()
    if missing:
        pytest.skip(f"{missing} is missing: the code objects cannot be read")
    kernels = {k["name"][5:]: k for k in kr.read(lib.path) if k["name"].startswith("hot::")}
    for name in NEW_KERNELS:
        assert name in kernels, name
        k = kernels[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    # the committed table is the built library's, and apart from the new rows it is the parent commit's: registers, spills, scratch and LDS
    # of every other kernel are where they were (compared with the table as git holds it at HEAD~ when the history is there)
    table = _table(open(os.path.join(ROOT, "profiles", "kernel_resources.txt")).read())
    for name in NEW_KERNELS:
        assert name in table, name
    built = {n: (k["vgpr"], k["agpr"], k["vgpr_spill"], k["scratch"], k["lds"]) for n, k in kernels.items()}
    assert built == table, {n: (built.get(n), table.get(n)) for n in set(built) | set(table) if built.get(n) != table.get(n)}
    # the kernels the V-cycle is made of, by name: spelled out so that the rule does not depend on git history being present
    pinned = {
        "k_vcycle_start<double>", "k_vcycle_start<float>", "k_apmv_sub<double>", "k_apmv_sub<float>", "k_spmv<double>", "k_spmv<float>",
        "k_cg_persist<double, 2>", "k_restrict<float>", "k_prolong<float>",
    }
    assert pinned <= set(table), pinned - set(table)
    r = subprocess.run(["git", "-C", ROOT, "log", "--format=%H", "-n", "40", "--", "profiles/kernel_resources.txt"], capture_output=True, text=True)
    commits = r.stdout.split() if r.returncode == 0 else []
    for rev in commits:  # every earlier version of the table that still knows no mg32 kernel: the parent's view
        old = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:profiles/kernel_resources.txt"], capture_output=True, text=True)
        if old.returncode != 0 or "k_mg32_" in old.stdout:
            continue
        before = _table(old.stdout)
        moved = {n: (before[n], table.get(n)) for n in before if table.get(n) != before[n]}
        assert not moved, moved
        assert set(table) - set(before) == set(NEW_KERNELS)
        break
