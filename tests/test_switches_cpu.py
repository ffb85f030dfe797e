"""The library's switch table (csrc/switches.h), without a GPU: defaults, the parsing rule of every variable, the read-only
query ffm_switch / ops.switch, and host queries that show the switches still act.

The table is read once per process, so every setting is a child process (`python <file> --child`) that prints what the
library answers; a setting is run once and shared by the tests that look at it.
"""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fairfedmed_amd", "csrc")

# variable -> default (FFM_PANEL_MASK_DEFAULT = bits 7, 8, 10; FFM_SKINNY_CAP / _NT / _MINB_DEFAULT = 0 / 2 / 1: csrc/switches.h)
DEFAULTS = {
    "FFM_PANEL": 0, "FFM_PANEL_MASK": 1408, "FFM_SKINNY": 0, "FFM_SKINNY_SPLITK": 2048, "FFM_SKINNY_SPLITK_MIN": 4,
    "FFM_SKINNY_CAP": 0, "FFM_SKINNY_NT": 2, "FFM_SKINNY_NT_NARROW": 2, "FFM_SKINNY_MINB": 1, "FFM_GEMM_DEEP": 1,
    "FFM_CONV_DEEP": 1, "FFM_CONV_NARROW": 0, "FFM_ATTN": 0, "FFM_ATTN_PARTS": 2, "FFM_ATTN3_MAP": 1,
    "FFM_BN_FOLD_ROWS": 32768, "FFM_BN_RPT": 2}

# (environment, what ffm_switch then answers for the variables named)
PARSING = [
    ({"FFM_PANEL": "off"}, {"FFM_PANEL": 1}),
    ({"FFM_PANEL": "0"}, {"FFM_PANEL": 1}),
    ({"FFM_PANEL": "on"}, {"FFM_PANEL": 0}),
    ({"FFM_SKINNY": "off"}, {"FFM_SKINNY": 1}),
    ({"FFM_SKINNY": "0"}, {"FFM_SKINNY": 0}),                        # (only `o` switches it off)
    ({"FFM_GEMM_DEEP": "0"}, {"FFM_GEMM_DEEP": 0}),
    ({"FFM_GEMM_DEEP": "1"}, {"FFM_GEMM_DEEP": 1}),
    ({"FFM_GEMM_DEEP": "off"}, {"FFM_GEMM_DEEP": 1}),                # (only `0` switches it off)
    ({"FFM_CONV_NARROW": "off"}, {"FFM_CONV_NARROW": -1}),
    ({"FFM_CONV_NARROW": "1000000"}, {"FFM_CONV_NARROW": 1000000}),
    ({"FFM_ATTN": "v1"}, {"FFM_ATTN": 1}),
    ({"FFM_ATTN": "v2"}, {"FFM_ATTN": 2}),
    ({"FFM_ATTN": "v3"}, {"FFM_ATTN": 3}),
    ({"FFM_ATTN": "v4"}, {"FFM_ATTN": 0}),
    ({"FFM_ATTN": "3"}, {"FFM_ATTN": 0}),
    ({"FFM_ATTN_PARTS": "4"}, {"FFM_ATTN_PARTS": 4}),
    ({"FFM_ATTN_PARTS": "2"}, {"FFM_ATTN_PARTS": 2}),
    ({"FFM_ATTN_PARTS": "8"}, {"FFM_ATTN_PARTS": 2}),
    ({"FFM_ATTN3_MAP": "0"}, {"FFM_ATTN3_MAP": 0}),
    ({"FFM_SKINNY_NT": "4"}, {"FFM_SKINNY_NT": 4, "FFM_SKINNY_NT_NARROW": 4}),      # (the narrow one follows the VALUE of the other)
    ({"FFM_SKINNY_NT": "4", "FFM_SKINNY_NT_NARROW": "1"}, {"FFM_SKINNY_NT": 4, "FFM_SKINNY_NT_NARROW": 1}),
    ({"FFM_PANEL_MASK": "7552"}, {"FFM_PANEL_MASK": 7552}),
    ({"FFM_BN_FOLD_ROWS": "0"}, {"FFM_BN_FOLD_ROWS": 0}),
    ({"FFM_BN_RPT": "4"}, {"FFM_BN_RPT": 4}),
]
LENGTHS = [96, 97, 197, 256, 257]


def child():
    sys.path.insert(0, ROOT)
    import torch
    from fairfedmed_amd import _lib as L
    from fairfedmed_amd import ops
    lib, v = L.load(), ctypes.c_int32(12345)
    out = {"switch": {name: ops.switch(name) for name in DEFAULTS},
           "splitk": ops.gemm_splitk_floats(40, 512, 2048),
           "lnstat": {str(dt).split(".")[1]: {str(n): ops.attention_bwd_lnstat_ok(n, False, dt) for n in LENGTHS}
                      for dt in (torch.bfloat16, torch.float16)},
           # an unknown name, a NULL value, a NULL name; `v` must stay untouched by all three
           "refused": [lib.ffm_switch(b"FFM_NO_SUCH_SWITCH", ctypes.byref(v)), lib.ffm_switch(b"FFM_PANEL", None),
                       lib.ffm_switch(None, ctypes.byref(v)), v.value]}
    try:
        ops.switch("ffm_panel")
        out["raised"] = False
    except RuntimeError:
        out["raised"] = True
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def _answers(setting):
    env = {k: v for k, v in os.environ.items() if k not in DEFAULTS}
    env.update(dict(setting), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def answers(**env):
    return _answers(tuple(sorted(env.items())))


def test_defaults():
    assert answers()["switch"] == DEFAULTS


@pytest.mark.parametrize("env,expect", PARSING, ids=[" ".join(f"{k}={v}" for k, v in e.items()) for e, _ in PARSING])
def test_parsing(env, expect):
    """One child per setting; every variable the setting does not name keeps its default.  (FFM_PANEL=on: the one value
    whose meaning the table changed - a first character `o` used to switch the panel kernel off, `on` included.)"""
    got = answers(**env)["switch"]
    want = dict(DEFAULTS, **expect)
    print(env, {k: got[k] for k in expect})
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_unknown_name_and_null_arguments_are_refused():
    a = answers()
    assert a["refused"] == [-1, -1, -1, 12345] and a["raised"]      # FFM_EINVAL; the names are the variables', case and all


def test_the_switches_still_act_on_host_queries():
    assert answers()["splitk"] > 0 and answers(FFM_SKINNY_SPLITK="0")["splitk"] == 0
    for dt in ("bfloat16", "float16"):                               # (float16 answers through the IEEE-half twin)
        assert answers()["lnstat"][dt] == {"96": False, "97": True, "197": True, "256": True, "257": False}, dt
        assert answers(FFM_ATTN="v3")["lnstat"][dt] == answers()["lnstat"][dt], dt
        for gen in ("v1", "v2"):
            assert not any(answers(FFM_ATTN=gen)["lnstat"][dt].values()), (gen, dt)


def test_one_place_reads_the_environment_and_every_variable_is_documented():
    readers = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".hpp", ".cpp", ".inc"))
               and "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["switches.hip"]
    table = open(os.path.join(CSRC, "switches.h")).read()
    rows = re.findall(r'^\s*X\(\s*\w+\s*,\s*"(FFM_\w+)"', table, re.M)
    assert sorted(rows) == sorted(DEFAULTS) and len(rows) == len(set(rows)) == 17
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in rows:
        assert re.search(rf"\b{name}\b", doc), f"{name} is not in INTEGRATION.md"
    assert "ffm_switch" in doc


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child()
