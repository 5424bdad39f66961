"""The tail rows the fused residual pass finishes (TransferTables::residual_tail_runs, csrc/transfer_tables.hpp), checked on the
host.  The fused 17-point bricks restrict their own partial sums and write neither t nor the tail accumulator, so the pass runs
its tail epilogue only over the set S of tail DoFs that a slot outside the fused set touches.  tools/residual_tail_check.cpp builds
S with the production function and checks, for every level with fused bricks: every tail entry in shell_idx of a non-fused slot is
in S (the accumulator entries somebody adds to), every tail DoF an un-fused patch restricts is in S (the rows of t somebody
reads), and S is a sorted list of disjoint runs inside [0, n_tail).  It prints |S| / n_tail per level."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"transfer (\d+) -> (\d+): (\d+) fused bricks, \|S\| = (\d+) of n_tail = (\d+) \(([0-9.]+)\) in (\d+) runs")


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "dealii_multigrid_amd", "csrc"),
                    os.path.join(ROOT, "tools", "residual_tail_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("residual_tail"), "residual_tail_check", ["-O2"])


def check(exe, geo, L, p):
    r = subprocess.run([exe, geo, str(L), str(p)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    levels = [LINE.search(l) for l in r.stdout.splitlines()]
    levels = [m for m in levels if m]
    assert levels and any(int(m.group(3)) > 0 for m in levels), r.stdout  # the case has fused bricks at all
    assert all("missing: 0 touched, 0 restricted, 0 malformed runs" in l for l in r.stdout.splitlines() if "fused bricks" in l)
    return [dict(n_fused=int(m.group(3)), size=int(m.group(4)), n_tail=int(m.group(5)), n_runs=int(m.group(7))) for m in levels]


# the annulus of tests/test_fuse_plan_host.py (bricks next to constrained cells, which stay un-fused): about 20 s
@pytest.mark.parametrize("geo,L,p", [("quadrant", 4, 4), ("quadrant", 6, 4), ("quadrant", 6, 1), ("hypercube", 3, 4), ("annulus", 8, 4)])
def test_residual_tail_rows_cover_what_is_read(checker, geo, L, p):
    levels = check(checker, geo, L, p)
    for lv in levels:
        assert lv["size"] <= lv["n_tail"]
    if geo == "hypercube":
        # every slot is a fused brick: nobody outside the fused set touches the tail
        assert all(lv["size"] == 0 and lv["n_runs"] == 0 for lv in levels)
    if (geo, L, p) == ("quadrant", 6, 4):
        # 343 fused bricks on the finest level: their common faces are NOT in S
        assert levels[0]["n_fused"] == 343 and 0 < levels[0]["size"] < 0.6 * levels[0]["n_tail"]
    if (geo, L, p) in (("quadrant", 4, 4), ("quadrant", 6, 1)):
        # one fused brick next to un-fused slots on three faces: S is the rim, here the whole tail
        assert levels[0]["n_fused"] == 1 and levels[0]["size"] > 0


def test_checker_under_sanitizers(tmp_path):
    exe = build(tmp_path, "residual_tail_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check(exe, "quadrant", 4, 4)
