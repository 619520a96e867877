"""The Python mirrors of the launch choosers (oracle/stream_cases.py, oracle/tshift_cases.py,
oracle/pw_cases.py, shiftgcn.ops.ra_fits / PW_MAX_ELEMS) against the C++ they restate
(shift-gcn_amd/csrc/launch_forms.hpp, pw_forms.hpp), without a GPU:
tests/launch_forms_dump.cpp prints the library's decision for every plane the mirrors'
reachable() enumerate and for every contraction size, its constants, and its form and tile
lists (the kernel instantiations the launchers build)."""
import itertools
import os
import subprocess

import pytest

from conftest import REPO
from oracle import pw_cases as pc
from oracle import stream_cases as sc
from oracle import tshift_cases as tc

HIPCC = "/opt/rocm/bin/hipcc"
N_MAX = sc.K_FWD_LDS_MAX2 + 2 * sc.K_PLANE_V_MAX

# the weight-gradient sizes asked of the C++ program: every M, Nc <= 300 on one plane (family
# and tile do not depend on it), then the split geometry on a grid of sizes around every
# tile and family edge x every plane of the test table and four more, then the table itself
PW_SIZES = range(1, 301)
DW_ENUM = [(2, M, Nc, 7, 25) for M in PW_SIZES for Nc in PW_SIZES]
DW_EDGES = (1, 3, 4, 5, 63, 64, 65, 100, 127, 128, 129, 200, 256, 257, 300)
DW_PLANES = sorted({(B, T, V) for B, _, _, T, V in pc.DW_TABLE} |
                   {(1, 1, 1), (2, 300, 25), (32, 75, 25), (64, 300, 33)})
DW_GRID = [(B, M, Nc, T, V) for B, T, V in DW_PLANES for M in DW_EDGES for Nc in DW_EDGES]
DW_QUERIES = DW_ENUM + DW_GRID + list(pc.DW_TABLE)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """The C++ program's lines by their first word (plane lines under "plane")."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = tmp_path_factory.mktemp("launch_forms") / "launch_forms_dump"
    src = os.path.join(REPO, "tests", "launch_forms_dump.cpp")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", src, "-o", str(exe)],
                   check=True)
    asked = "".join("%d %d %d %d %d\n" % q for q in DW_QUERIES)
    out = subprocess.run([str(exe)], input=asked, check=True, capture_output=True,
                         text=True).stdout
    by = {k: [] for k in ("const", "list", "tile", "pwfwd", "pwtsh", "pwdw", "plane")}
    for line in out.splitlines():
        by.get(line[:line.index(" ")], by["plane"]).append(line)
    return by


@pytest.fixture(scope="module")
def dump(printed):
    """(form lists {name: {(nt, lpt)}}, plane lines) printed by the C++ program."""
    lists = {}
    for line in printed["list"]:
        _, name, nt, lpt = line.split()
        assert (int(nt), int(lpt)) not in lists.setdefault(name, set()), line
        lists[name].add((int(nt), int(lpt)))
    return lists, printed["plane"]


def _line(chooser, H, W, arg, form, flag=0):
    """One line of the dump from a mirror's return value."""
    if form in ("refuse", "empty"):
        kind, nt, lpt = form, 0, 0
    elif form == "loop":
        kind, nt, lpt = form, tc.K_THREADS, 0
    elif form[0] == "global":                       # (.., per-thread, loops)
        kind, nt, lpt, flag = "global", tc.K_THREADS, form[-2], form[-1]
    elif form[0] == "s2":                           # (s2, per-thread, joint-aligned)
        kind, nt, lpt, flag = "s2", tc.K_BWD_THREADS, form[1], form[2]
    else:                                           # (kind, threads, per-thread[, down])
        kind, nt, lpt = form[:3]
        kind = "lds" if kind == "fallback" else kind
    return f"{chooser} {H} {W} {arg} {kind} {nt} {lpt} {int(flag)}"


def _mirror_lines():
    for V in range(1, sc.K_PLANE_V_MAX + 2):
        for T in range(1, N_MAX // V + 2):
            yield _line("bn", T, V, 0, sc.bn_form(T, V))
            yield _line("fused", T, V, 0, sc.fwd_form(T, V))
            yield _line("bnin", T, V, 0, sc.bnin_form(T, V))
    for W in range(1, 131):
        for H in range(1, N_MAX // W + 2):
            for stride in (1, 2):
                yield _line("fwd", H, W, stride, tc.fwd_form(H, W, stride))
                yield _line("bwd", H, W, stride, tc.bwd_form(H, W, stride))
            for down in (0, 1):
                yield _line("gbn", H, W, down, tc.gbn_form(H, W, down), flag=down)


def test_mirrors_agree_with_the_library_on_every_plane(dump):
    _, planes = dump
    want = list(_mirror_lines())
    assert len(planes) == len(want) > 300000
    bad = [(got, exp) for got, exp in zip(planes, want) if got != exp]
    assert not bad, (len(bad), bad[:5])
    kinds = {(p.split()[0], p.split()[4]) for p in planes}
    assert {("bn", "refuse"), ("fused", "refuse"), ("bnin", "refuse"), ("gbn", "refuse"),
            ("fwd", "empty")} <= kinds


def test_ra_fits_agrees_with_the_library(dump):
    """ops.ra_fits (pure Python) accepts exactly the planes sgcn_tshift_bwd_bnin launches."""
    from shiftgcn import ops
    n = 0
    for p in dump[1]:
        if p.startswith("bnin "):
            _, H, W, _, kind = p.split()[:5]
            assert ops.ra_fits(int(H) * int(W), int(W)) == (kind != "refuse"), p
            n += 1
    assert n > 100000


# form list -> the (chooser, argument, kind) whose launcher instantiates it
LIST_USERS = {
    "kJaForms": [("bn", 0, "ja")],
    "kPadFwdForms": [("fused", 0, "pad"), ("fwd", 1, "pad"), ("fwd", 2, "pad")],
    "kLdsFwdForms": [("fused", 0, "lds"), ("fwd", 1, "lds"), ("fwd", 2, "lds")],
    "kRaForms": [("bwd", 1, "ra"), ("gbn", 0, "ra")],
    "kGbdForms": [("gbn", 1, "ra")],
    "kBninForms": [("bnin", 0, "ra")],
}


def test_form_lists_are_exactly_the_reachable_forms(dump):
    """No dead instantiation, and no reachable form the dispatcher would refuse."""
    lists, planes = dump
    assert set(lists) == set(LIST_USERS)
    seen = {}
    for p in planes:
        chooser, _, _, arg, kind, nt, lpt, _ = p.split()
        seen.setdefault((chooser, int(arg), kind), set()).add((int(nt), int(lpt)))
    for name, users in LIST_USERS.items():
        for user in users:
            assert seen[user] == lists[name], (name, user)
    # every (nt, lpt) kind of every chooser is behind a list (global / s2 / loop are not:
    # one thread count, the per-thread count an enumerated flag)
    listed = {u for users in LIST_USERS.values() for u in users}
    assert {k for k in seen if k[2] in ("ja", "pad", "lds", "ra")} == listed
    # the lists of the issue, literally
    assert lists["kJaForms"] == ({(256, l) for l in (8, 16, 24, 32)} | {(512, 24), (512, 32)})
    assert lists["kPadFwdForms"] == ({(256, l) for l in (8, 16, 24, 32)} |
                                     {(512, l) for l in (20, 24, 32)})
    assert lists["kBninForms"] == ({(256, l) for l in (8, 16, 24)} |
                                   {(512, l) for l in (12, 16, 20, 24, 32)})
    # and they are what the mirrors reach
    assert {("ja",) + f for f in lists["kJaForms"]} == sc.reachable(sc.bn_form) - {"loop"}
    assert ({("ra",) + f for f in lists["kRaForms"]} ==
            {f for f in tc.reachable(lambda H, W: tc.bwd_form(H, W, 1)) if f[0] == "ra"})
    assert ({("ra",) + f + (True,) for f in lists["kGbdForms"]} ==
            tc.reachable(lambda H, W: tc.gbn_form(H, W, True)))


# --------------------------------------------------------------------------------------
# the contraction choosers (pw_forms.hpp) against oracle/pw_cases.py
# --------------------------------------------------------------------------------------
def _same(got, want):
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (len(bad), bad[:5])


def _fwd_lines():
    for M in PW_SIZES:
        for K in range(1, pc.K_MAX_K + 1):
            for mask, xr, yr in itertools.product((0, 1), repeat=3):
                fam, tile, stage, _ = pc.fwd_form(M, K, bool(mask), xr, yr)
                bm, bn = tile or (0, 0)
                yield f"pwfwd {M} {K} {mask} {xr} {yr} {fam} {bm} {bn} {int(stage == 'ar')}"


def test_forward_mirrors_agree_with_the_library_on_every_size(printed):
    _same(printed["pwfwd"], list(_fwd_lines()))
    assert len(printed["pwfwd"]) == 300 * 256 * 8
    _same(printed["pwtsh"], ["pwtsh %d %d %d" % ((M,) + pc.tshift_form(M)) for M in PW_SIZES])


def _dw_mirror(B, M, Nc, T, V, ws_bytes=None):
    """The mirror's whole weight-gradient decision, as the C++ program prints it."""
    f = pc.dw_form(B, M, Nc, T, V)
    ws = f["S"] * (M * Nc + M) * 4 if ws_bytes is None else ws_bytes(B, M, Nc, T, V)
    if f["family"] == "smallc":
        bm, bn, bkp = 4 * pc.K_DWC_ROWS, Nc, 64
    else:
        (bm, bn), bkp = f["tile"], pc.dw3_cfg(M, Nc)[2] if f["family"] == "dw3" else pc.K_DW_BK
    tiles = -(-M // bm) * -(-Nc // bn)
    return (f"pwdw {B} {M} {Nc} {T} {V} {f['family']} {bm} {bn} {bkp} {tiles} {f['S']} "
            f"{f['per']} {ws} {int(pc.use_dwc(Nc))} "
            f"{int(pc.use_dw3(M, Nc))}")


def test_weight_gradient_mirrors_agree_with_the_library(printed):
    """Family, tile, use_dwc and use_dw3 on every M, Nc <= 300; those and the split count,
    chunks per split and workspace bytes on the geometry grid and on every row of the test
    table."""
    got = printed["pwdw"]
    assert [tuple(int(x) for x in g.split()[1:6]) for g in got] == DW_QUERIES
    _same(got, [_dw_mirror(*q) for q in DW_ENUM] +
          [_dw_mirror(*q, ws_bytes=pc.dw_ws_bytes) for q in DW_QUERIES[len(DW_ENUM):]])
    assert len(DW_GRID) == 15 * 15 * len(DW_PLANES) and len(DW_PLANES) >= 12
    assert {g.split()[6] for g in got[len(DW_ENUM):]} == {"smallc", "dw3", "dw"}


def test_constants_agree_with_the_library(printed):
    from shiftgcn import ops
    consts = {name: int(v) for _, name, v in (line.split() for line in printed["const"])}
    assert consts == {
        "kSmallM": pc.K_SMALL_M, "kDwBK": pc.K_DW_BK, "kDwcRows": pc.K_DWC_ROWS,
        "kDwcMaxC": pc.K_DWC_MAX_C, "SGCN_DW3_MIN": pc.K_DW3_MIN,
        "SGCN_DW3_BKP_BIG": pc.K_DW3_BKP_BIG, "kMaskMaxV": pc.K_MASK_MAX_V,
        "kPwMaxK": pc.K_MAX_K, "kPwMaxElems": pc.K_EXTENT}
    assert ops.PW_MAX_ELEMS == consts["kPwMaxElems"]


def test_tile_lists_are_exactly_the_reachable_tiles(printed):
    """No dead instantiation, and no reachable tile the dispatcher would refuse: each tile
    list is the set of tiles its chooser returns over the enumeration."""
    tiles = {}
    for line in printed["tile"]:
        name, *t = line.split()[1:]
        tiles.setdefault(name, []).append(tuple(int(x) for x in t))
    assert all(len(set(v)) == len(v) for v in tiles.values())
    tiles = {k: set(v) for k, v in tiles.items()}
    # the lists of the issue, literally: (bm, bn, wm, wn, A-resident | positions per chunk)
    big = pc.K_DW3_BKP_BIG
    assert tiles == {
        "kPwFwdTiles": {(64, 256, 2, 4, 0), (64, 256, 2, 4, 1), (128, 128, 4, 2, 0),
                        (256, 128, 4, 2, 0)},
        "kPwTshTiles": {(64, 256, 2, 4, 0), (128, 256, 2, 4, 0), (256, 128, 4, 2, 0)},
        "kDw3Tiles": {(128, 128, 2, 2, 16), (256, 128, 4, 2, big), (256, 256, 4, 2, big)},
        "kDwTiles": {(bm, bn, bm // 32, 2, pc.K_DW_BK) for bm in (64, 128) for bn in (64, 128)},
        "kDwcForms": {(1,), (2,), (3,), (4,)}}
    # what the choosers return (the lines carry bm, bn and ar | bkp: the waves follow the tile)
    fwd = {tuple(int(x) for x in p.split()[7:]) for p in printed["pwfwd"] if " pwg " in p}
    assert fwd == {(bm, bn, x) for bm, bn, _, _, x in tiles["kPwFwdTiles"]}
    tsh = {tuple(int(x) for x in p.split()[2:]) for p in printed["pwtsh"]}
    assert tsh == {t[:2] for t in tiles["kPwTshTiles"]} and len(tsh) == 3
    dw = {}
    for p in printed["pwdw"][:len(DW_ENUM)]:
        w = p.split()
        dw.setdefault(w[6], set()).add((int(w[7]), int(w[8]), int(w[9])))
    assert dw["dw3"] == {(bm, bn, bkp) for bm, bn, _, _, bkp in tiles["kDw3Tiles"]}
    assert dw["dw"] == {(bm, bn, bkp) for bm, bn, _, _, bkp in tiles["kDwTiles"]}
    assert {(bn,) for _, bn, _ in dw["smallc"]} == tiles["kDwcForms"]
