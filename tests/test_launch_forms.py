"""The Python mirrors of the launch choosers (oracle/stream_cases.py, oracle/tshift_cases.py,
shiftgcn.ops.ra_fits) against the C++ they restate (shift-gcn_amd/csrc/launch_forms.hpp),
without a GPU: tests/launch_forms_dump.cpp prints the library's decision for every plane the
mirrors' reachable() enumerate, and its form lists (the kernel instantiations the launchers
build)."""
import os
import subprocess

import pytest

from conftest import REPO
from oracle import stream_cases as sc
from oracle import tshift_cases as tc

HIPCC = "/opt/rocm/bin/hipcc"
N_MAX = sc.K_FWD_LDS_MAX2 + 2 * sc.K_PLANE_V_MAX


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """(form lists {name: {(nt, lpt)}}, plane lines) printed by the C++ program."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = tmp_path_factory.mktemp("launch_forms") / "launch_forms_dump"
    src = os.path.join(REPO, "tests", "launch_forms_dump.cpp")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", src, "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lists, planes = {}, []
    for line in out.splitlines():
        if line.startswith("list "):
            _, name, nt, lpt = line.split()
            assert (int(nt), int(lpt)) not in lists.setdefault(name, set()), line
            lists[name].add((int(nt), int(lpt)))
        else:
            planes.append(line)
    return lists, planes


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
