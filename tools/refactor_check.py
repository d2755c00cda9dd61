#!/usr/bin/env python3
"""Has a refactor of sp_coupler_amd/csrc/ left the GPU work alone?  Compares two builds of libspc_hip.so, no GPU needed:
 A. the gfx950 code object, per kernel symbol: the disassembly and the kernel's entry in the code-object metadata (registers,
    spills, LDS, scratch, kernarg layout).  Per symbol, because the file as a whole differs between builds that only move text.
 B. the text of spc_describe_launch over CUs x geometries x pitches x shared grid x cols_per_block x columns x passes x
    element sizes (168 960 calls), by default and under each environment switch the tests use.
 C. the seven spc_les_*_cols_per_block exports (the column tile of spc_coltile.hpp) for ktot 0 ... 4096 and element sizes 2, 4, 8.
Exit status 1 on any difference.
--touched SUBSTRING[,SUBSTRING...]: a kernel symbol that contains one of the substrings may differ in its disassembly; its
instruction count and whether both builds use the same multiset of mnemonics are printed, and its metadata entry must still
be identical.  Every other symbol must be identical as before.
usage: python tools/refactor_check.py OLD.so NEW.so [--touched k_a,k_b] > profiles/<change>.log"""
import collections
import ctypes
import hashlib
import importlib.util
import itertools
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
spec = importlib.util.spec_from_file_location("_abi", os.path.join(ROOT, "sp_coupler_amd", "_abi.py"))   # not the package: no torch
_abi = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_abi)

CUS = (32, 64, 128, 256, 304)
GEOS = ((91, 160), (137, 512), (19, 160), (60, 128), (91, 400), (91, 2000))
COLS = (1, 16, 255, 256, 257, 512, 513, 1024, 1025, 1100, 2048, 2560, 3072, 4096, 8192, 16384, 25000, 25001, 35718, 88838,
        174264, 348528)
PASSES = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0), (4, 0))
SWITCHES = ({}, {"SPC_SMALL_BLOCK": "0"}, {"SPC_K1_PRE": "0"}, {"SPC_K1_PRE": "1"}, {"SPC_F32_VEC": "0"})


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def code_object(lib, tmp):
    """({symbol: disassembly}, {kernel: metadata entry}) of the gfx950 code object in `lib`"""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "rest"))
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
        "--input=" + fat, "--output=" + co)
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    parts = re.split(r"^<([^>\n]+)>:\n", text, flags=re.M)
    dis = {name: re.sub(r"[ \t]*//.*$", "", body, flags=re.M) for name, body in zip(parts[1::2], parts[2::2])}
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    kernels = notes.split("amdhsa.kernels:\n", 1)[1].split("\namdhsa.", 1)[0]
    meta = {re.search(r"\.name: +(\S+)", e).group(1): e for e in re.split(r"^  - ", kernels, flags=re.M)[1:]}
    return dis, meta


def launches(lib_path, env):
    """every spc_describe_launch text of the cross product under the environment `env`, one per line"""
    for k in ("SPC_SMALL_BLOCK", "SPC_K1_PRE", "SPC_F32_VEC"):
        os.environ.pop(k, None)
    os.environ.update(env)
    # (only what is called here is bound: the old build of a change that adds an entry point does not export it)
    lib, out = _abi.bind(ctypes.CDLL(lib_path), {k: _abi.PROTOTYPES[k] for k in ("spc_describe_launch", "spc_last_error")}), []
    for cus in CUS:
        os.environ["SPC_CUS"] = str(cus)
        for (nG, nL), pad, shared, cb, n, (pass_, flags), es in itertools.product(GEOS, (0, 1), (0, 1), (0, 1, 2, 8), COLS, PASSES, (8, 4)):
            d = _abi.Dims(n, nG, nL, nG + pad, nG + 1 + pad, nL + pad, shared, cb)
            buf = ctypes.create_string_buffer(256)
            rc = lib.spc_describe_launch(ctypes.byref(d), pass_, flags, es, buf, len(buf))
            out.append(buf.value.decode() if rc >= 0 else "error %d: %s" % (rc, lib.spc_last_error().decode()))
    return out


COLS_EXPORTS = ("diffuse", "vadvect", "transport", "transport2", "radiate", "buoyancy", "vmix")


def mnemonics(body):
    """the mnemonic of every instruction of a symbol's disassembly (labels and blank lines left out)"""
    return [line.split()[0] for line in body.splitlines() if line.strip() and not line.rstrip().endswith(":")]


def cols_per_block(lib_path):
    lib = ctypes.CDLL(lib_path)
    return [getattr(lib, "spc_les_%s_cols_per_block" % k)(ktot, es) for k in COLS_EXPORTS for es in (2, 4, 8) for ktot in range(4097)]


def main(old, new, touched=()):
    bad = moved = 0
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        (dis_o, meta_o), (dis_n, meta_n) = code_object(old, t1), code_object(new, t2)
    for what, o, n in (("disassembly", dis_o, dis_n), ("metadata", meta_o, meta_n)):
        only = sorted(set(o) ^ set(n))
        differ = sorted(k for k in set(o) & set(n) if o[k] != n[k])
        allowed = [k for k in differ if what == "disassembly" and any(t in k for t in touched)]
        print("A %s: %d symbols old, %d new, %d on one side only, %d differ, %d of them touched" % (what, len(o), len(n), len(only), len(differ), len(allowed)))
        for k in only + differ:
            if k in allowed:
                mo, mn = mnemonics(o[k]), mnemonics(n[k])
                print("   TOUCHED  %s: %d instructions old, %d new, mnemonic multiset %s" % (
                    k, len(mo), len(mn), "equal" if collections.Counter(mo) == collections.Counter(mn) else "DIFFERS"))
            else:
                print("   %s %s" % ("ONE SIDE" if k in only else "DIFFERS ", k))
        bad += len(only) + len(differ) - len(allowed)
        moved += len(allowed)
    for env in SWITCHES:
        o, n = launches(old, env), launches(new, env)
        diff = [i for i, (a, b) in enumerate(zip(o, n)) if a != b]
        names = {line.split(" ")[0] for line in n}
        print("B %-20s %d calls, %d errors, %d distinct instantiations, sha256 old %s new %s, %d differ" % (
            " ".join("%s=%s" % kv for kv in env.items()) or "default", len(n), sum(line.startswith("error") for line in n), len(names),
            hashlib.sha256("\n".join(o).encode()).hexdigest()[:16], hashlib.sha256("\n".join(n).encode()).hexdigest()[:16], len(diff)))
        for i in diff[:10]:
            print("   call %d\n     old %s\n     new %s" % (i, o[i], n[i]))
        bad += len(diff) + (len(o) != len(n))
    o, n = cols_per_block(old), cols_per_block(new)
    diff = sum(a != b for a, b in zip(o, n))
    print("C cols_per_block: %d exports, %d calls, %d differ" % (len(COLS_EXPORTS), len(n), diff))
    bad += diff
    print("refactor_check: %s" % ("FAILED, %d differences" % bad if bad else "identical" + (" but for the disassembly of %d touched kernels" % moved if moved else "")))
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    touched = ()
    if "--touched" in args:
        i = args.index("--touched")
        touched = tuple(t for t in args[i + 1].split(",") if t)
        del args[i:i + 2]
    sys.exit(main(args[0], args[1], touched))
