"""CPU-side checks of the per-particle plasticity classes (include/hot_mi355x.h hot_set_plasticity_classes): the boundary is
declared, exported and mirrored, the ABI version did not move, and the class kernel k_g2p<T, 3, true> came out of the compiler without scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hot_amd
from hot_amd import binding, kernel_resources as kr, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hot_set_plasticity_classes", "hot_get_plasticity_classes", "hot_plasticity_eval_classes")


def _header():
    return open(os.path.join(ROOT, "include", "hot_mi355x.h")).read()


def test_header_declares_the_class_boundary():
    hdr = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*hot_ctx\s*\*" % name, hdr), name
    m = re.search(r"typedef struct hot_plasticity_class \{(.*?)\} hot_plasticity_class;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int32_t kind", "int32_t reserved", "double yield_stress", "double snow[5]"], fields
    assert re.search(r"#define HOT_ABI_VERSION 7\b", hdr)
    for name in NAMES:  # HIP product only: the CPU checker is loaded through the same binding and does not export them
        assert name[4:] in hot_amd.PRODUCT_ONLY_SYMBOLS and name[4:] not in hot_amd.ABI_SYMBOLS


def test_library_exports_the_class_boundary():
    if not os.path.exists(hot_amd.LIB_PATH):
        hot_amd.build()
    lib = hot_amd.load()
    for name in NAMES:
        assert hasattr(lib.lib, name), name
    assert lib.fn["abi_version"]() == 7 == hot_amd.binding.ABI_VERSION
    for meth in ("set_plasticity_classes", "plasticity_classes", "plasticity_eval_classes"):
        assert callable(getattr(hot_amd.Context, meth))


def test_struct_mirror_is_56_bytes():
    s = binding.hot_plasticity_class
    assert C.sizeof(s) == 56
    assert (s.kind.offset, s.reserved.offset, s.yield_stress.offset, s.snow.offset) == (0, 4, 8, 16)
    assert C.sizeof(binding.hot_config) == C.sizeof(hot_amd.hot_config)  # (untouched: no field of hot_config or hot_stats changed)


def test_class_kernels_have_no_scratch():
    if not os.path.exists(hot_amd.LIB_PATH):
        hot_amd.build()
    missing = kr.tools_missing()
    if missing:
        pytest.skip(f"{missing} is missing: the code objects cannot be read")
    kernels = {k["name"]: k for k in kr.read(hot_amd.LIB_PATH)}
    for name in ("hot::k_g2p<double, 3, true>", "hot::k_g2p<float, 3, true>"):
        assert name in kernels, name
        k = kernels[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    # the kernels of hot_config.plasticity keep what they had (profiles/kernel_resources.txt): the class kernel is an overload beside them, not a change to them
    assert kernels["hot::k_g2p<double, 0, true>"]["scratch"] == 0 and kernels["hot::k_g2p<double, 0, true>"]["vgpr"] <= 160
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.txt")).read()
    for name in ("k_g2p<double, 3, true>", "k_g2p<float, 3, true>", "k_plasticity_eval_classes<double>"):
        assert re.search(r"^%s\s" % re.escape(name), table, flags=re.M), name


def test_two_body_cloud():
    c = synth.two_body_cloud(8)
    n = len(c["X"])
    assert all(len(c[k]) == n for k in ("V", "mass", "vol", "mu", "lam", "cls")) and c["cls"].dtype == np.int32
    ball, block = c["cls"] == 1, c["cls"] == 0
    assert [d["kind"] for d in c["classes"]] == [2, 0] and len(c["classes"][0]["snow"]) == 5
    ext = (c["X"][block].max(0) - c["X"][block].min(0)) / c["dx"]
    assert np.allclose(ext, (16, 8, 8), atol=0.2)  # the reference block's 2 : 1 : 1
    r = 0.5 * (c["X"][ball].max(0) - c["X"][ball].min(0)) / c["dx"]
    assert np.allclose(r, 2.0, atol=0.25)  # radius = a quarter of the block's height
    gap = (c["X"][ball][:, 1].min() - c["X"][block][:, 1].max()) / c["dx"]
    assert 1.5 < gap < 2.5  # the ball hangs one radius above the block
    assert np.unique(c["mu"][ball]).size == 1 and c["mu"][ball][0] / c["mu"][block][0] == pytest.approx(1e8 / 1.4e5)
    assert not np.array_equal(c["cls"], np.sort(c["cls"]))  # shuffled caller order
