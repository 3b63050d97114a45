"""The relaxation kernels (csrc/mm_relax_kernels.hip, the seeded search of csrc/mm_tri_kernels.hip, csrc/mm_relax.cpp) on
the worst cases of tests/relax_attack_cases.py: ties between a face and its copy in another chunk, query blocks carried
across chunks in one step, a block whose box one vertex stretches over the whole reference, offsets of 2^20 and 2^36,
scales of 2^-200, 2^200 and 2^600, previous faces that are degenerate, thin or give a NaN, and the exact grid.

(a) every case equals the unpruned scan of tests/mm_checkers/relax_mesh.py bit for bit (same_relax of
    tests/test_gpu_relax.py: vertices, ref_face, the integer and f64 fields of the report, launches, bytes, items);
(b) (c) (d) the device's own output goes through check_result of tests/test_relax_attack_host.py: the exact oracle of
    tests/relax_exact.py is asked about what the device returned, not about the checker;
(e) the iterations skip at least the items that must be skipped (skip_claim there), and (a) proves none was skipped
    wrongly;
(f) a large offset, the ties and a tiny mesh through one engine give what fresh engines give.

With step 0's bounds kept for the iterations (k_relax_candidates not storing the refreshed lb2), tried on an MI355X,
ten tests here fail -- (a) on stale_up, stale_down_twice, the four tie cases with iterations and seed_needle_axis, (e)
on both stale cases, and (f) -- while tests/test_gpu_relax.py passes."""
import numpy as np
import pytest

import relax_attack_cases as AC
from test_gpu_relax import same_relax, settled
from test_refine_host import same_bits
from test_relax_attack_host import SKIP_FAMILIES, arrays, check_result, checked, free_of, skip_claim
from test_trim_host import octahedron

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu


def run(engine, name):
    v, f, rv, rf, pinned, iterations, lamb = arrays(AC.cases()[name])
    reference = None if AC.cases()[name][2] is None else (rv, rf)
    return same_relax((v, f), reference, engine, iterations, lamb, pinned=pinned, want=checked(name))


@pytest.mark.parametrize("name", AC.NAMES)
def test_attack_cases_equal_the_unpruned_scan_and_lie_on_the_surface(engine, name):
    x, face, rep = run(engine, name)                                      # (a)
    worst = check_result(name, x, face, rep)                              # (b) (c) (d)
    print(f"{name}: worst on-surface ratio {worst:.3f} of the bound; {rep['items_run']} items run, "
          f"{rep['items_skipped']} skipped, {rep['items_skipped_step0']} of them at step 0")
    assert worst <= 1.0
    if AC.cases()[name][4] == 0:                                          # project_to_mesh is the same call
        v, f, rv, rf, pinned, _, _ = arrays(AC.cases()[name])
        (pv, _), pface, prep = mm.project_to_mesh((v, f), (rv, rf), pinned=pinned, engine=engine)
        assert same_bits(pv, x) and np.array_equal(pface, face) and settled(prep) == settled(rep)


@pytest.mark.parametrize("name", [n for n in AC.NAMES if AC.family(n) in SKIP_FAMILIES and AC.cases()[n][4] > 0])
def test_iterations_skip_what_they_must(engine, name):
    plan, counts, _ = skip_claim(name)                                    # (e)
    iterations = AC.cases()[name][4]
    _, _, rep = run(engine, name)
    n_items = len(plan["a"]) + len(plan["b"])
    later = rep["items_skipped"] - rep["items_skipped_step0"]
    print(f"{name}: {n_items} items a pass; step 0 skipped {rep['items_skipped_step0']}, the iterations {later}, "
          f"must skip {counts}")
    assert rep["items_run"] + rep["items_skipped"] == n_items * (1 + iterations)
    assert later >= sum(counts) and rep["items_skipped_step0"] <= len(plan["b"])
    if AC.family(name) == "stale":
        assert sum(counts) > 0


@pytest.mark.parametrize("name", ["wide_8", "wide_64"])
def test_one_thrown_vertex_changes_no_other_result(engine, name):
    v, f, rv, rf, pinned, iterations, lamb = arrays(AC.cases()[name])
    x, face, rep = run(engine, name)
    held = pinned.copy()
    held[AC.ROGUE[name]] = True                                           # the same mesh with R held: 511 free vertices
    (hv, _), hface, hrep = mm.relax_mesh((v, f), (rv, rf), iterations=iterations, lamb=lamb, pinned=held, engine=engine)
    others = free_of(name).copy()
    others[AC.ROGUE[name]] = False
    assert hrep["n_free"] == 511 == int(others.sum())
    assert same_bits(x[others], hv[others]) and np.array_equal(face[others], hface[others])


def test_one_engine_several_calls(engine):
    """(f): scratch carried from a call at 2^36 or from the ties into the next call would show here."""
    names = ("offset_2p36", "ties_3", "scale_2m200")
    tiny = octahedron()
    fresh = []
    for name in names:
        with mm.Engine() as one:
            fresh.append(run(one, name))
    with mm.Engine() as one:
        (tv, _), tface, trep = mm.relax_mesh(tiny, iterations=2, engine=one)
    with mm.Engine() as shared:
        for _ in range(2):
            for name, (x, face, rep) in zip(names, fresh):
                gx, gface, grep = run(shared, name)
                assert same_bits(gx, x) and np.array_equal(gface, face) and settled(grep) == settled(rep)
            (gv, _), gface, grep = mm.relax_mesh(tiny, iterations=2, engine=shared)
            assert same_bits(gv, tv) and np.array_equal(gface, tface) and settled(grep) == settled(trep)
