"""sgcn_pw_fwd_bf16 without a GPU: the Python mirror of its chooser (tests/bf16_cases.py)
against the C++ it restates (pw_forms.hpp, through tests/bf16_forms_dump.cpp), the tile list
against what the chooser can return, the symbol's declaration / export / ctypes binding, the
argument checks (nothing is launched), and the precision setting's host-side behaviour."""
import os
import subprocess
import sys

import pytest

import bf16_cases as bc
from conftest import PKG_ROOT, REPO

HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(M, K) for M in range(1, 301) for K in range(1, bc.K_MAX_K + 1)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = tmp_path_factory.mktemp("bf16_forms") / "bf16_forms_dump"
    src = os.path.join(REPO, "tests", "bf16_forms_dump.cpp")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", src, "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    by = {"const": [], "tile": [], "pwbf16": []}
    for line in out.splitlines():
        by[line[:line.index(" ")]].append(line)
    return by


def test_constants(printed):
    consts = dict(line.split()[1:] for line in printed["const"])
    assert int(consts["kPwBf16BK"]) == bc.K_BF16_BK
    assert int(consts["kPwMaxK"]) == bc.K_MAX_K
    from shiftgcn import ops
    assert int(consts["kSmallM"]) == ops.SMALL_M


def test_mirror_equals_the_chooser_on_every_size(printed):
    want = ["pwbf16 %d %d %d %d %d %d" % ((M, K) + bc.bf16_form(M, K)) for M, K in SIZES]
    assert printed["pwbf16"] == want


def test_tile_list_is_exactly_what_the_chooser_returns(printed):
    tiles = [tuple(int(v) for v in line.split()[2:]) for line in printed["tile"]]
    assert tiles == bc.BF16_TILES and len(set(tiles)) == len(tiles)
    reached = {tuple(int(v) for v in line.split()[3:]) for line in printed["pwbf16"]}
    assert reached == set(tiles)
    # the test tables reach every tile, and each with K mod 32 in {0, 1, 31}
    for tile in tiles:
        ms = [M for M in bc.BF16_MS if bc.bf16_form(M, 1) == tile]
        assert ms and {K % 32 for K in bc.BF16_KS} >= {0, 1, 31}
        assert bc.bf16_form(*bc.BF16_FLAG_PAIRS[tile[:2]]) == tile
        assert bc.bf16_form(*bc.BF16_EXACT[tile[:2]]) == tile


def test_symbol_declared_exported_and_bound():
    from shiftgcn import _lib
    from test_capi import declared_symbols
    assert "sgcn_pw_fwd_bf16" in declared_symbols()
    lib = _lib.load()
    assert hasattr(lib, "sgcn_pw_fwd_bf16")
    res, args = _lib.SIGNATURES["sgcn_pw_fwd_bf16"]
    assert len(args) == 19 and lib.sgcn_pw_fwd_bf16.argtypes == args
    assert lib.sgcn_abi_version() == _lib.ABI_VERSION == 25


def _call(lib, w=64, x=64, y=64, w_mcontig=0, bias=None, xb=1000, xc=50, xt=1, yb=1000, yc=50,
          yt=1, yr=0, relu=0, B=2, M=8, K=8, T=2, V=25):
    return lib.sgcn_pw_fwd_bf16(w, w_mcontig, bias, x, xb, xc, xt, y, yb, yc, yt, yr, relu, B, M,
                                K, T, V, None)


def test_bad_arguments_rejected_before_any_launch():
    """Every call below returns from the argument checks: no launch, no GPU needed (the
    pointers are never dereferenced on the host)."""
    from shiftgcn import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    assert _call(lib, w=None) == E and _call(lib, x=None) == E and _call(lib, y=None) == E
    assert _call(lib, K=257) == E and _call(lib, K=0) == E and _call(lib, M=0) == E
    assert _call(lib, yr=2) == E and _call(lib, yr=-2) == E
    assert _call(lib, xt=0) == E and _call(lib, yt=0) == E
    assert _call(lib, xb=1 << 29) == E and _call(lib, yb=1 << 29) == E   # past kPwMaxElems
    assert _call(lib, B=-1) == E and _call(lib, V=0) == E
    # B == 0 (and T == 0) return 0 without a launch, null pointers or not
    assert _call(lib, B=0) == 0 and _call(lib, B=0, w=None, x=None, y=None) == 0
    assert _call(lib, T=0) == 0


def test_precision_setting_host_side():
    import threading

    import shiftgcn
    from shiftgcn import fused
    assert shiftgcn.eval_precision is fused.eval_precision
    base = fused.current_eval_precision()
    with pytest.raises(ValueError):
        fused.eval_precision("int8")
    with fused.eval_precision("bf16"):
        assert fused.current_eval_precision() == "bf16"
        with fused.eval_precision("fp32"):
            assert fused.current_eval_precision() == "fp32"
        assert fused.current_eval_precision() == "bf16"
        seen = []
        t = threading.Thread(target=lambda: seen.append(fused.current_eval_precision()))
        t.start()
        t.join()
        assert seen == [fused.EVAL_PRECISION]          # thread-local: other threads keep theirs
    assert fused.current_eval_precision() == base


@pytest.mark.parametrize("value,ok", [("bf16", True), ("fp32", True), (None, True),
                                      ("int8", False)])
def test_environment_default(value, ok):
    env = {k: v for k, v in os.environ.items() if k != "SGCN_EVAL_PRECISION"}
    if value is not None:
        env["SGCN_EVAL_PRECISION"] = value
    env["PYTHONPATH"] = PKG_ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "from shiftgcn import fused; print(fused.EVAL_PRECISION, fused.current_eval_precision())"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr
        assert r.stdout.split() == [value or "fp32"] * 2
    else:
        assert r.returncode != 0 and "ValueError" in r.stderr
