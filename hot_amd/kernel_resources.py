"""What the compiler gave every kernel of a built library: registers, spills, scratch, LDS — read from the gfx950 code objects inside the
shared library with the two LLVM tools of the ROCm install (no GPU needed).  tools/kernel_resources.py prints the table,
tests/test_kernel_resources.py keeps the product kernels free of scratch."""
import os
import re
import shutil
import subprocess
import tempfile

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
OBJDUMP = os.path.join(LLVM_BIN, "llvm-objdump")
READELF = os.path.join(LLVM_BIN, "llvm-readelf")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

_FIELDS = {
    "agpr": "agpr_count", "vgpr": "vgpr_count", "sgpr": "sgpr_count", "vgpr_spill": "vgpr_spill_count", "sgpr_spill": "sgpr_spill_count",
    "scratch": "private_segment_fixed_size", "lds": "group_segment_fixed_size", "max_threads": "max_flat_workgroup_size",
}
_BUILTIN = {"d": "double", "f": "float", "i": "int", "j": "unsigned", "b": "bool", "h": "unsigned char", "t": "unsigned short", "l": "long", "m": "unsigned long"}


def tools_missing():
    """Name of the first LLVM tool that is not there, or None."""
    for t in (OBJDUMP, READELF):
        if not os.path.exists(t):
            return t
    return None


def short_name(symbol):
    """`hot::k_gs_sweep<double, true, 64, true>` from the Itanium symbol of a kernel whose template arguments are builtin types and literals
    (all of this library's are); a symbol outside that subset comes back unchanged, and so does one of another namespace."""
    m = re.match(r"_ZN3hot(\d+)", symbol)
    if not m:
        return symbol
    n, at = int(m.group(1)), m.end()
    name, rest = symbol[at:at + n], symbol[at + n:]
    if not rest.startswith("I"):
        return "hot::" + name
    args, i = [], 1
    while i < len(rest) and rest[i] != "E":
        if rest[i] in _BUILTIN:
            args.append(_BUILTIN[rest[i]])
            i += 1
            continue
        lit = re.match(r"L([a-z])(n?)(\d+)E", rest[i:])
        if not lit:
            return symbol
        ty, neg, val = lit.groups()
        args.append(("true" if val != "0" else "false") if ty == "b" else ("-" if neg else "") + val)
        i += lit.end()
    return "hot::%s<%s>" % (name, ", ".join(args))


def waves_per_simd(vgpr, agpr=0):
    """Wavefronts per SIMD the register file allows: 512 registers per lane, allocated in granules of 8, at most 8 wavefronts."""
    alloc = max(8, -(-(vgpr + agpr) // 8) * 8)
    return min(8, 512 // alloc)


def read(lib_path):
    """One dict per kernel of the gfx950 images inside lib_path: symbol, name, vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, scratch (bytes per lane),
    lds (static bytes), max_threads, waves_per_simd (by registers, capped by max_threads).  A kernel compiled into several images is listed once."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, copy)
        subprocess.run([OBJDUMP, "--offloading", copy], check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        images = sorted(f for f in os.listdir(tmp) if f.endswith(TARGET))
        if not images:
            raise RuntimeError("%s holds no %s image" % (lib_path, TARGET))
        for img in images:
            notes = subprocess.run([READELF, "--notes", os.path.join(tmp, img)], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"^\s*- (?=\.agpr_count:)", notes, flags=re.M)[1:]:
                sym = re.search(r"^\s*\.symbol:\s+(\S+)", blk, flags=re.M)
                if not sym:
                    continue
                k = {"symbol": sym.group(1)[:-3] if sym.group(1).endswith(".kd") else sym.group(1)}
                for key, field in _FIELDS.items():
                    m = re.search(r"^\s*\.%s:\s+(\d+)" % field, blk, flags=re.M)
                    k[key] = int(m.group(1)) if m else 0
                k["name"] = short_name(k["symbol"])
                # a workgroup of max_threads must fit a compute unit's four SIMDs: its wavefronts per SIMD are a floor as well as the registers' ceiling
                k["waves_per_simd"] = waves_per_simd(k["vgpr"], k["agpr"])
                prev = out.get(k["symbol"])
                if prev is None or (k["scratch"], k["vgpr_spill"], k["vgpr"]) > (prev["scratch"], prev["vgpr_spill"], prev["vgpr"]):
                    out[k["symbol"]] = k
    return sorted(out.values(), key=lambda k: k["name"])
