"""The hierarchy policy of the library (include/mgamd.h, "Hierarchy policy"; no GPU): which (mesh, degree) pairs form the levels of
every multigrid type, what a coarse solver needs next to the levels, which coarse solver then runs, and the defaults of the two-tier
partition.  The harness, the C++ layer and the Python hierarchies all build what these functions say."""
import ctypes as C
import itertools

import pytest

PLAIN, NESTED, SHARDED_AMG = 0, 1, 2


@pytest.mark.parametrize("mg_type,n_meshes,degree,levels,local_smoothing", [
    ("HMG-global", 4, 4, [(0, 4), (1, 4), (2, 4), (3, 4)], False),
    ("PMG", 1, 4, [(0, 1), (0, 2), (0, 4)], False),
    ("PMG", 4, 4, [(3, 1), (3, 2), (3, 4)], False),  # sharded: the partition's mesh sequence, p-levels on its finest mesh
    ("HPMG", 4, 4, [(0, 1), (1, 1), (2, 1), (3, 1), (3, 2), (3, 4)], False),
    ("HPMG", 1, 4, [(0, 1), (0, 2), (0, 4)], False),
    ("HPMG", 3, 1, [(0, 1), (1, 1), (2, 1)], False),
    ("HMG-local", 4, 4, [(0, 4), (1, 4), (2, 4), (3, 4)], True),
    ("HMG-local", 1, 2, [(0, 2)], True),
    ("HPMG-local", 1, 4, [(0, 1), (0, 2), (0, 4)], False),  # the HMG-local plan at degree 1 underneath is the caller's
    ("HPMG-local", 1, 1, [(0, 1)], False),
])
def test_level_plan(mgamd, mg_type, n_meshes, degree, levels, local_smoothing):
    assert mgamd._level_plan(mg_type, n_meshes, degree) == (levels, local_smoothing)


@pytest.mark.parametrize("p,seq", [(1, [1]), (2, [1, 2]), (3, [1, 3]), (4, [1, 2, 4]), (5, [1, 2, 5]), (6, [1, 3, 6]), (7, [1, 3, 7])])
def test_degree_sequences(mgamd, p, seq):
    assert [d for _, d in mgamd._level_plan("PMG", 1, p)[0]] == seq
    assert [d for _, d in mgamd._level_plan("HPMG", 3, p)[0]] == [seq[0]] * 3 + seq[1:]
    assert list(mgamd.create_polynomial_coarsening_sequence(p)) == seq


@pytest.mark.parametrize("mg_type", ["AMG", "AMGPETSc", "HMG", ""])
def test_types_without_levels_are_refused(mgamd, mg_type):
    n, ls, mesh, deg = C.c_uint(), C.c_int(), (C.c_uint * 8)(), (C.c_uint * 8)()
    assert mgamd._lib.mgamd_level_plan(mg_type.encode(), 3, 2, 8, C.byref(n), mesh, deg, C.byref(ls)) == 1  # MGAMD_ERR
    assert mgamd._lib.mgamd_last_error().decode() == f"Type '{mg_type}': not implemented"
    with pytest.raises(mgamd.MgamdError, match="not implemented"):
        mgamd._level_plan(mg_type, 3, 2)


def test_level_plan_checks_its_room(mgamd):
    n, ls, mesh, deg = C.c_uint(), C.c_int(), (C.c_uint * 8)(), (C.c_uint * 8)()
    assert mgamd._lib.mgamd_level_plan(b"HPMG", 6, 4, 7, C.byref(n), mesh, deg, C.byref(ls)) == 3  # MGAMD_ERR_INVALID: 8 levels
    assert mgamd._lib.mgamd_level_plan(b"HPMG", 6, 4, 8, C.byref(n), mesh, deg, C.byref(ls)) == 0 and n.value == 8
    assert mgamd._lib.mgamd_level_plan(b"PMG", 0, 4, 8, C.byref(n), mesh, deg, C.byref(ls)) == 3


# above the exact solve's limit, by (level 0 distributed, sharded AMG requested) = (no, no), (no, yes), (yes, no), (yes, yes)
ABOVE = {"amg": (PLAIN, SHARDED_AMG, NESTED, SHARDED_AMG), "cg_with_amg": (PLAIN, SHARDED_AMG, NESTED, SHARDED_AMG),
         "amg_petsc": (PLAIN, SHARDED_AMG, NESTED, SHARDED_AMG), "gmg_vcycle": (NESTED, NESTED, NESTED, NESTED),
         "cg": (PLAIN, PLAIN, PLAIN, PLAIN), "cg_with_chebyshev": (PLAIN, PLAIN, PLAIN, PLAIN)}


@pytest.mark.parametrize("name", sorted(ABOVE))
def test_coarse_plan(mgamd, name):
    for i, (distributed, requested) in enumerate(itertools.product((False, True), repeat=2)):
        assert mgamd._coarse_plan(name, 4096, distributed, requested) == PLAIN, (distributed, requested)
        assert mgamd._coarse_plan(name, 4097, distributed, requested) == ABOVE[name][i], (distributed, requested)
    assert (mgamd.COARSE_PLAIN, mgamd.COARSE_NESTED, mgamd.COARSE_SHARDED_AMG) == (PLAIN, NESTED, SHARDED_AMG)


# What a multigrid RUNS (mgamd_debug_coarse_resolve): coarse_solver_used(), or the error of its construction.  Errors, by the texts
# the library raises (status: 3 MGAMD_ERR_INVALID, 1 MGAMD_ERR):
ERRORS = {
    "G": (3, "multigrid: the sharded algebraic multigrid takes the place of the AMG coarse solvers (amg, cg_with_amg, amg_petsc) and "
             "excludes a nested multigrid"),
    "N": (3, "multigrid: a nested multigrid is the stand-in for the AMG coarse solvers only"),
    "S": (1, "CoarseGridSolverType '{name}' on a sharded coarse level: the algebraic multigrid is built from one rank's assembled "
             "matrix; use the nested geometric multigrid (gmg_vcycle), cg or cg_with_chebyshev"),
    "V": (3, "multigrid: CoarseGridSolverType 'gmg_vcycle' on a level of more than 4096 DoFs needs a nested multigrid"),
    "U": (3, "CoarseGridSolverType '{name}' not implemented"),
}
# name -> (at 4096 DoFs, at 4097 DoFs) for (sharded, nested, amg_global) =
#         (0,0,0)                   (0,0,1)                         (0,1,0)                       (0,1,1)
#         (1,0,0)                   (1,0,1)                         (1,1,0)                       (1,1,1)
RESOLVE = {
    "amg": [("direct", "amg"), ("amg", "amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G"),
            ("direct", "S"), ("amg", "amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G")],
    "amg_petsc": [("direct", "amg"), ("amg", "amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G"),
                  ("direct", "S"), ("amg", "amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G")],
    "cg_with_amg": [("direct", "cg_with_amg"), ("cg_with_amg", "cg_with_amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G"),
                    ("direct", "S"), ("cg_with_amg", "cg_with_amg"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G")],
    "gmg_vcycle": [("direct", "V"), ("G", "G"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G"),
                   ("direct", "V"), ("G", "G"), ("gmg_vcycle", "gmg_vcycle"), ("G", "G")],
    "direct": [("direct", "direct"), ("G", "G"), ("N", "N"), ("G", "G"),
               ("direct", "direct"), ("G", "G"), ("N", "N"), ("G", "G")],
    "cg": [("cg", "cg"), ("G", "G"), ("N", "N"), ("G", "G"),
           ("cg", "cg"), ("G", "G"), ("N", "N"), ("G", "G")],
    "cg_with_chebyshev": [("cg_with_chebyshev", "cg_with_chebyshev"), ("G", "G"), ("N", "N"), ("G", "G"),
                          ("cg_with_chebyshev", "cg_with_chebyshev"), ("G", "G"), ("N", "N"), ("G", "G")],
    "ilu": [("U", "U"), ("G", "G"), ("N", "N"), ("G", "G"),
            ("U", "U"), ("G", "G"), ("N", "N"), ("G", "G")],
}


@pytest.mark.parametrize("name", sorted(RESOLVE))
def test_coarse_resolve(mgamd, name):
    for i, (sharded, nested, amg_global) in enumerate(itertools.product((False, True), repeat=3)):
        for n_dofs, expected in zip((4096, 4097), RESOLVE[name][i]):
            case = (n_dofs, sharded, nested, amg_global)
            used = C.create_string_buffer(32)
            status = mgamd._lib.mgamd_debug_coarse_resolve(name.encode(), C.c_uint64(n_dofs), int(sharded), int(nested), int(amg_global), used)
            if expected in ERRORS:
                code, text = ERRORS[expected]
                assert status == code, case
                assert mgamd._lib.mgamd_last_error().decode() == text.format(name=name), case
                with pytest.raises(mgamd.MgamdError):
                    mgamd._coarse_resolve(name, *case)
            else:
                assert status == 0 and used.value.decode() == expected, case
                assert mgamd._coarse_resolve(name, *case) == expected, case


def test_partition_defaults(mgamd):
    ranks = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16]
    assert [mgamd._partition_defaults(n)[0] for n in ranks] == [1, 1, 1, 2, 1, 2, 1, 4, 2, 4, 4]
    assert mgamd._partition_defaults(8, 1)[1:] == (4_000_000, 1_000_000)
    assert mgamd._partition_defaults(8, 2)[1:] == (500_000, 125_000)
    assert mgamd._partition_defaults(8, 4)[1:] == (62_500, 15_625)
    assert (mgamd.MIN_ROOT_DOFS_DEFAULT, mgamd.MIN_SUBSET_DOFS_DEFAULT) == (4_000_000, 1_000_000)
