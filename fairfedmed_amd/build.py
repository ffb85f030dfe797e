"""Build libffm_hip.so (gfx950) in-tree with hipcc.

    python -m fairfedmed_amd.build [--force]

hipcc cross-compiles without a GPU.  Objects are rebuilt only when their source
(or a header) is newer, so repeated calls cost nothing.

Two storage types share one set of 16-bit kernel sources (bfloat16 and IEEE half, the reference's PREC="fp16"): every
file in TWIN_SOURCES is compiled twice - once as written (float32 + bfloat16, entry points renamed ``<name>_m``) and once
with ``-DFFM_TWIN_F16`` (csrc/common.h: the file's 16-bit type becomes _Float16; every external symbol renamed
``<name>_f16``) - and a generated translation unit (csrc/_gen_dispatch.hip, from the prototypes of include/ffm_hip.h)
defines the public entry points that take a ``dtype``: FFM_F16 goes to the half twin, everything else to the main object.
A twin holds 16-bit kernels only: the storage-type dispatch of csrc/common.h (ffm_by_storage) names no float kernel there.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(CSRC, "libffm_hip.so")
SOURCES = ["gemm.hip", "gemm_panel.hip", "gemm_panel_rk.hip", "gemm_panel_rk2.hip", "gemm_panel_rk3.hip", "gemm_skinny.hip", "rowwise.hip", "lora.hip", "head.hip", "head_ot.hip", "optim.hip", "dp.hip", "drift.hip", "attention.hip", "attention3.hip", "attention_long.hip", "slice3d.hip", "conv.hip", "evalmetrics.hip", "evalsort.hip", "evalboot.hip", "transport.hip", "resize.hip", "augment.hip", "text.hip", "switches.hip"]
# files with 16-bit kernels behind a `dtype` argument (attention3.hip and attention_long.hip are templated on the storage types and need no
# twin; switches.hip has no kernels: the one switch table, csrc/switches.h, that the main objects and the twins both read)
TWIN_SOURCES = ["gemm.hip", "gemm_panel.hip", "gemm_panel_rk.hip", "gemm_panel_rk2.hip", "gemm_panel_rk3.hip", "gemm_skinny.hip", "rowwise.hip", "lora.hip", "head.hip", "head_ot.hip", "attention.hip", "slice3d.hip", "conv.hip"]
# C++-linkage names shared between those files (csrc/gemm_panel.h): renamed in the twins with the entry points
TWIN_INTERNAL = ["ffm_panel", "ffm_panel_select", "ffm_panel_launch", "ffm_panel_launch_rk",
                 "ffm_panel_launch_rk2", "ffm_panel_launch_rk3", "ffm_skinny_ok", "ffm_skinny_launch"]
HEADER = os.path.join(ROOT, "include", "ffm_hip.h")
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "gemm_panel.h"), os.path.join(CSRC, "gemm_panel_impl.h"), os.path.join(CSRC, "switches.h"), os.path.join(CSRC, "evalkeys.h"), os.path.join(CSRC, "philox.h"), HEADER]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# per-source extras.  attention3.hip: row maxima over MFMA results - without nnan hipcc puts a canonicalising
# v_max_f32 x, x in front of every fmaxf operand (200 v_max for 112 scores per lane; 85 with it); the kernels mask with
# -inf selects and never produce or consume a NaN
# slice3d.hip: the fp32 convolution passes keep their weights in SGPRs (v_fmac_f32 v, s, v); the SLP vectoriser pairs the
# FMAs into v_pk_fma_f32 on register pairs, copies the weights into VGPRs for that and spills (1 KB of scratch per lane)
EXTRA_FLAGS = {"attention3.hip": ["-fno-honor-nans"], "slice3d.hip": ["-fno-slp-vectorize"]}
GEN_MAIN, GEN_TWIN, GEN_DISPATCH = (os.path.join(CSRC, n) for n in ("_gen_rename_main.h", "_gen_rename_f16.h", "_gen_dispatch.hip"))


def _hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the FairLoRA HIP library cannot be built")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def api_prototypes():
    """[(return type, name, [(type, name), ...])] of every function include/ffm_hip.h declares."""
    s = open(HEADER).read()
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    s = re.sub(r"//[^\n]*", "", s)
    out = []
    for rt, name, args in re.findall(r"\n\s*(int|void|const char\s*\*)\s+(ffm_\w+)\s*\(([^;{}]*?)\)\s*;", s):
        params = []
        a = " ".join(args.split())
        if a and a != "void":
            for p in a.split(","):
                m = re.match(r"^(.*?)(\w+)$", p.strip())
                params.append((m.group(1).strip(), m.group(2)))
        out.append((rt, name, params))
    return out


def _write_if_changed(path: str, text: str) -> None:
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)


def generate() -> None:
    """The two rename headers and the dispatcher (regenerated whenever the public header changes; not tracked)."""
    protos = api_prototypes()
    typed = [p for p in protos if any(n == "dtype" for _, n in p[2])]
    note = "// generated by fairfedmed_amd/build.py from include/ffm_hip.h - do not edit\n"
    _write_if_changed(GEN_MAIN, note + "".join(f"#define {n} {n}_m\n" for _, n, _ in typed))
    _write_if_changed(GEN_TWIN, note + "".join(f"#define {n} {n}_f16\n" for n in [p[1] for p in protos] + TWIN_INTERNAL))
    body = [note, '#include "../../include/ffm_hip.h"\n', 'extern "C" {\n']
    for rt, n, params in typed:
        sig = ", ".join(f"{t} {a}" for t, a in params)
        body.append(f"{rt} {n}_m({sig});\n{rt} {n}_f16({sig});\n")
    for rt, n, params in typed:
        sig = ", ".join(f"{t} {a}" for t, a in params)
        call = ", ".join(a for _, a in params)
        body.append(f"{rt} {n}({sig}) {{ return dtype == FFM_F16 ? {n}_f16({call}) : {n}_m({call}); }}\n")
    body.append("}\n")
    _write_if_changed(GEN_DISPATCH, "".join(body))


def build(force: bool = False, verbose: bool = True, stamps: bool = False) -> str:
    """stamps=True: the diagnostic twin libffm_hip_stamps.so whose panel GEMM writes in-kernel phase time stamps
    (tools/panel_stamps.py); every other object is shared with the product build."""
    hipcc = _hipcc()
    generate()
    objs, jobs = [], []
    lib = LIB.replace(".so", "_stamps.so") if stamps else LIB
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        special = stamps and (src.startswith("gemm_panel") or src == "lora.hip")
        o = os.path.join(CSRC, src.replace(".hip", ".stamps.o" if special else ".o"))
        objs.append(o)
        if force or _stale(o, [s, GEN_MAIN] + HEADERS) or (special and os.environ.get("FFM_STAMPS_DEFS")):
            extra = ["-DFFM_PANEL_STAMPS"] + os.environ.get("FFM_STAMPS_DEFS", "").split() if special else []
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + extra + ["-include", GEN_MAIN, "-c", s, "-o", o])
    for src in TWIN_SOURCES:                               # the IEEE-half twins (never stamped)
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".f16.o"))
        objs.append(o)
        if force or _stale(o, [s, GEN_TWIN] + HEADERS):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-DFFM_TWIN_F16", "-include", GEN_TWIN, "-c", s, "-o", o])
    o = GEN_DISPATCH.replace(".hip", ".o")
    objs.append(o)
    if force or _stale(o, [GEN_DISPATCH, HEADER]):
        jobs.append([hipcc] + FLAGS + ["-c", GEN_DISPATCH, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{r.stdout}\n{r.stderr}")
        return r

    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(lib, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", "-o", lib] + objs)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, stamps="--stamps" in sys.argv))
