"""The geodesic field and the band skeleton on the device (csrc/mm_geodesic_kernels.hip, csrc/mm_geodesic.cpp) on the worst
cases of tests/geo_attack_cases.py: hubs whose rows of 7 to 300 entries cross every block of 256 vertices, a hub that
falls a second time and alone can flag a block, detours whose vertices fall up to 199 times, weights over 60 binades, in
the subnormal range, all zero and at the top of the range, and band skeletons at the edges of the bitonic sort, with
everything in one node, with 599 edges between two nodes and with plain means beyond block 0.

(a) every field case equals the checker bit for bit (same_field of tests/test_gpu_skeleton.py: dist, pred, the counts;
    1 <= rounds <= nv + 1);
(b) the device's own dist and pred go through check_field of tests/test_geo_attack_host.py: the exact oracle of
    tests/geo_exact.py is asked about what the device returned, not about the checker;
(c) every band case equals the checker (same_skeleton), and the device's vertex_node, node integers and node edges equal
    the breadth-first search of tests/geo_exact.py over the device's own dist;
(d) the largest band case, hub_seed_300, a detour, an all-zero case and a mesh of five vertices through one engine give
    what fresh engines give;
(e) the largest detour twice on one engine: the same bits, whatever the rounds.

No case here found a fault in the kernel or the host schedule.  Two mutants of k_geo_round, tried on an MI355X:

(i)  without the loop over the row entries from the ninth on, fourteen tests here fail -- (a) on all five late_out and all
     five late_in hubs and on the three permuted detours (the seed's row of 40 to 100 entries; detour_in_order passes),
     and (c) on bands_hub_one_node -- and tests/test_gpu_skeleton.py notices too: wound_tube_vertex (a cap centre of
     valence 15) and both soups fail.
(ii) with the publishing loop flagging only the blocks of the first eight entries, hub_meet_17, hub_meet_64 and
     hub_meet_300 fail (a), dist against the checker (the cases built so that only the hub can flag one block when it
     falls for the second time), and every other test here
     and every field, soup and skeleton-soup test of tests/test_gpu_skeleton.py passes: the old file cannot see it."""
import numpy as np
import pytest

import geo_attack_cases as AC
from test_geo_attack_host import check_field, check_partition, checked
from test_gpu_skeleton import NODE_FLOATS, NODE_INTS, same_field, same_skeleton
from test_refine_host import same_bits

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", AC.FIELD_NAMES)
def test_field_cases_equal_the_checker_and_the_exact_field(engine, name):
    _, v, f, seeds = AC.cases()[name]
    rep = same_field(v, f, seeds, checked(name), engine)                  # (a)
    dist, pred, _ = mm.mesh_geodesic_distance((v, f), seeds, engine=engine)
    worst = check_field(name, dist, pred)                                # (b)
    print(f"{name}: {rep['rounds']} rounds in {rep['n_batches']} batches; worst |dist - D| / (D u) = {worst:.2f} of at most about "
          f"{len(v) - 1}")


@pytest.mark.parametrize("name", AC.BANDS_NAMES)
def test_band_cases_equal_the_checker_and_the_search(engine, name):
    _, v, f, seeds, band = AC.cases()[name]
    got, _ = same_skeleton(v, f, seeds, band, engine)                    # (c)
    k, m = check_partition(name, got.dist, got.vertex_node, got.nodes, got.edges)
    assert (k, m) == (got.report["n_nodes"], got.report["n_node_edges"])
    if name in AC.BANDS_EXPECT:
        assert (k, m) == AC.BANDS_EXPECT[name]
    print(f"{name}: {k} nodes, {m} node edges, {got.report['union_rounds']} union rounds, {got.report['n_launches']} launches")


def five_vertices():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [1.5, 1.0, 0.0], [2.0, 0.0, 0.25]])
    return v, np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]], dtype=np.int64), np.array([4], dtype=np.int64), 0.75


def skeleton_of(name, engine):
    _, v, f, seeds, band = AC.cases()[name] if name != "five" else ("five",) + five_vertices()
    return mm.mesh_skeleton((v, f), seeds, band_mm=band, engine=engine)


def field_of(name, engine):
    _, v, f, seeds = AC.cases()[name]
    return mm.mesh_geodesic_distance((v, f), seeds, engine=engine)[:2]


def same_graph(a, b):
    assert same_bits(a.dist, b.dist) and np.array_equal(a.pred, b.pred) and np.array_equal(a.vertex_node, b.vertex_node)
    assert len(a.nodes) == len(b.nodes) and np.array_equal(a.edges, b.edges)
    for k in NODE_FLOATS:
        assert same_bits(a.nodes[k], b.nodes[k]), k
    for k in NODE_INTS:
        assert np.array_equal(a.nodes[k], b.nodes[k]), k


def test_one_engine_several_calls():
    """(d): flags, marks, the field or a sort buffer carried from a large call into the next would show here."""
    largest = max(AC.BANDS_NAMES, key=lambda n: len(AC.cases()[n][1]))
    assert largest == "bands_nodes_4097"
    fields = ("hub_seed_300", "detour_3_blocks", "weights_2m600_grid")
    with mm.Engine() as one:
        first = skeleton_of(largest, one)
    fresh = []
    for name in fields:
        with mm.Engine() as one:
            fresh.append(field_of(name, one))
    with mm.Engine() as one:
        last = skeleton_of("five", one)
    with mm.Engine() as shared:
        for _ in range(2):
            same_graph(skeleton_of(largest, shared), first)
            for name, (dist, pred) in zip(fields, fresh):
                got_dist, got_pred = field_of(name, shared)
                assert same_bits(got_dist, dist) and np.array_equal(got_pred, pred), name
            same_graph(skeleton_of("five", shared), last)


def test_the_largest_detour_twice(engine):
    """(e): the schedule is free, the bits are not."""
    _, v, f, seeds = AC.cases()["detour_5_blocks"]
    a_dist, a_pred, a = mm.mesh_geodesic_distance((v, f), seeds, engine=engine)
    b_dist, b_pred, b = mm.mesh_geodesic_distance((v, f), seeds, engine=engine)
    print(f"detour_5_blocks: {a['rounds']} and {b['rounds']} rounds")
    assert same_bits(a_dist, b_dist) and np.array_equal(a_pred, b_pred)
    assert 1 <= a["rounds"] <= len(v) + 1 and 1 <= b["rounds"] <= len(v) + 1
