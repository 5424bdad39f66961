"""The harness key "ShardedAMG" (this project's extension, default false): with MGAMD_HARNESS_SHARDED=1 the JSON-driven binary runs
the sharded code path on the one real RCCL rank a one-GPU box can run (RCCL refuses two ranks on one device); with "ShardedAMG":
true the AMG coarse solvers go through the sharded algebraic multigrid (mgamd_mg_create_sharded_amg: setup from the global tables,
gather / scatter between the level-0 vector and the AMG rows) and the table says so."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "dealii_multigrid_amd", "bin", "multigrid_throughput")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def final_table(stdout):
    lines = stdout.rstrip().split("\n")
    start = max(i for i, l in enumerate(lines) if l.startswith("dim "))
    header = lines[start].split()
    return header, [dict(zip(header, l.split())) for l in lines[start + 1:] if l.strip()]


@pytest.mark.parametrize("coarse,n_cycles", [("amg", 2), ("cg_with_amg", 1)])
def test_sharded_amg_key_with_one_rank_over_rccl(tmp_path, coarse, n_cycles):
    """PMG annulus L=6 p=2 (9,763-DoF coarse level): the `coarse_solver` column names the AMG, the note line says what runs, and the
    iteration counts equal the unsharded harness run"""
    assert os.path.exists(BIN), "build the harness with `make` (__graft_entry__.build())"
    base = json.load(open(os.path.join(GOLDEN, "input_0003.json")))
    cfg = dict(base, Type="PMG", GeometryType="annulus", NRefGlobal=6, Degree=2, MGNumberType="double", CoarseSolverNCycles=n_cycles,
               CoarseGridSolverType=coarse)
    f = str(tmp_path / "plain.json")
    json.dump(cfg, open(f, "w"))
    r = subprocess.run([BIN, f], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _, plain = final_table(r.stdout)
    assert plain[0]["coarse_solver"] == coarse
    fs = str(tmp_path / "sharded_amg.json")
    json.dump(dict(cfg, ShardedAMG=True), open(fs, "w"))
    env = dict(os.environ, MGAMD_HARNESS_SHARDED="1", MGAMD_RCCL_ID_FILE=str(tmp_path / "rccl_id"), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([BIN, fs], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    _, sharded = final_table(r.stdout)
    assert sharded[0]["coarse_solver"] == coarse
    assert "smoothed-aggregation AMG, rows cut over the ranks" in r.stdout
    for key in ("n_cells", "n_dofs", "n_levels", "n_iterations", "sub_comm_size"):
        assert sharded[0][key] == plain[0][key], key
