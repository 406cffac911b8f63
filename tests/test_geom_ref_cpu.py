"""tests/geom_ref.py on a machine without a GPU: the plain reference agrees with oracle/ops.py (two statements of the contract that were
written separately), every named case of tests/test_gpu_geom_kernels.py meets the condition its name claims (planted pairs in rational
arithmetic), and every wrong kernel restated as a variant of the reference changes the cases it is stated to change - and none of the
cases it is stated to spare.  Every comparison is an exact integer or bit comparison."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import geom_ref as R

F = np.float32


# ---- the reference against oracle/ops.py -----------------------------------------------------------------------------------------------

def _clouds():
    rng = np.random.default_rng(1)
    uniform = [rng.uniform(0, 1, (n, 3)) for n in (300, 1, 170)]
    u = rng.normal(size=(400, 3))
    surface = [u / np.linalg.norm(u, axis=1, keepdims=True) * 0.4, rng.uniform(-0.4, 0.4, (90, 3))]
    base = rng.uniform(0, 1, (80, 3))
    duplicate = [np.concatenate([base, base, base[:20]]), base[:50]]
    lattice = [np.stack(np.meshgrid(*[np.arange(6) * 0.125] * 3, indexing="ij"), -1).reshape(-1, 3), np.zeros((0, 3)),
               np.stack(np.meshgrid(*[np.arange(4) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)]
    return {"uniform": uniform, "surface": surface, "duplicate": duplicate, "lattice": lattice}


CLOUDS = _clouds()


def _flat(parts):
    parts = [np.asarray(v, F).reshape(-1, 3) for v in parts]
    P, ptr = np.concatenate(parts), R._ptr([len(v) for v in parts])
    batch = np.repeat(np.arange(len(parts)), [len(v) for v in parts])
    return P, ptr, batch


def _edges(nbr, deg):
    """(query, candidate) pairs of a neighbour table, query-major in slot order."""
    q, s = np.nonzero(np.arange(nbr.shape[1])[None, :] < deg[:, None])
    return np.stack([q, nbr[q, s]]).astype(np.int64)


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("res", [0.04, 0.125, 0.3])
def test_sampler_equals_oracle_voxel_grid_and_consecutive_cluster(cloud, res):
    P, ptr, batch = _flat(CLOUDS[cloud])
    S = R.sample(R.records(P, np.zeros(len(P), np.int32)), ptr, res)
    cell = O.voxel_grid(torch.from_numpy(P), res, torch.from_numpy(batch))
    assert np.array_equal(cell.numpy().astype(np.uint64), S.keys)
    inv, perm = O.consecutive_cluster(cell)
    assert np.array_equal(inv.numpy(), S.inv) and np.array_equal(perm.numpy(), S.idx)
    assert np.array_equal(S.sorted_keys, np.sort(S.keys)) and np.array_equal(S.keys[S.order], S.sorted_keys)
    assert np.array_equal(S.cell_keys, S.keys[S.idx]) and np.array_equal(S.rank_sorted, S.inv[S.order])
    assert np.array_equal(S.batch, batch[S.idx]) and np.array_equal(np.diff(S.ptr), np.bincount(S.batch, minlength=len(ptr) - 1))


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("k", [1, 3, 16, 70])
def test_knn_equals_oracle(cloud, k):
    P, ptr, batch = _flat(CLOUDS[cloud])
    Q, ptr_q, batch_q = _flat([v[::2] + 0.01 for v in CLOUDS[cloud]])
    nbr, deg = R.knn(R.records(P, np.zeros(len(P), np.int32)), ptr, R.records(Q, np.zeros(len(Q), np.int32)), ptr_q, k)
    want = O.knn(torch.from_numpy(P), torch.from_numpy(Q), k, torch.from_numpy(batch), torch.from_numpy(batch_q))
    assert np.array_equal(_edges(nbr, deg), want.numpy())


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("r,cap", [(0.08, 32), (0.25, 4), (0.125, 64), (0.6, 100)])
def test_ball_equals_oracle(cloud, r, cap):
    P, ptr, batch = _flat(CLOUDS[cloud])
    Q, ptr_q, batch_q = _flat([v[::2] for v in CLOUDS[cloud]])
    nbr, deg = R.ball(R.records(P, np.zeros(len(P), np.int32)), ptr, R.records(Q, np.zeros(len(Q), np.int32)), ptr_q, r, cap)
    want = O.radius(torch.from_numpy(P), torch.from_numpy(Q), r, torch.from_numpy(batch), torch.from_numpy(batch_q), max_num_neighbors=cap)
    assert np.array_equal(_edges(nbr, deg), want.numpy())
    assert ((nbr >= 0) == (np.arange(cap)[None, :] < deg[:, None])).all() and (nbr[nbr < 0] == -1).all()


def test_rational_rounding_equals_numpy_float32():
    rng = np.random.default_rng(2)
    q, c = rng.uniform(-2, 2, (300, 3)).astype(F), rng.uniform(-2, 2, (300, 3)).astype(F)
    for form in ("sum", "reassoc"):
        got = R.d2_rows(q, c, form)
        assert all(Fraction(float(got[i])) == R.exact_d2(q[i], c[i], form) for i in range(300))
    for v in (1 / 3, 0.1, 1e-20, 3e20, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24)):
        assert R.rnd32(Fraction(v)) == Fraction(float(F(v)))


# ---- every named case meets its condition ------------------------------------------------------------------------------------------

def _where(c, p):
    """Storage position of the candidate with coordinates p."""
    hit = np.flatnonzero((c.x[:, :3] == np.asarray(p, F)).all(1))
    assert len(hit) == 1
    return int(hit[0])


def _w(c):
    return c.x[:, 3].view(np.int32)


PAIRS = sorted(R.planted_pairs())


def test_every_predicate_pair_was_found():
    assert len(PAIRS) == 11 and R.planted_radius() is not None


@pytest.mark.parametrize("pair", PAIRS)
def test_predicate_pair_in_rational_arithmetic_and_in_its_cloud(pair):
    q, p = R.planted_pairs()[pair]
    assert R._confirm(pair, q, p, R.R_BALL)
    c = R.search_case("ball_" + pair)
    assert np.array_equal(c.q[0, :3], q)
    pos = _where(c, p)
    inside = R.exact_d2(q, p) < Fraction(float(R.r2_of(R.R_BALL)))
    for flags, ident in ((0, pos), (R.X_INDEX_IN_W, int(_w(c)[pos]))):
        nbr, deg = R.ball(c.x, c.ptr_x, c.q, c.ptr_q, R.R_BALL, 32, flags)
        assert deg[0] < 32 and (ident in nbr[0].tolist()) == inside


def test_radius_case_separates_the_two_squares():
    r, q, p = R.planted_radius()
    a, b = Fraction(float(R.r2_of(r))), Fraction(float(R.r2_f32(r)))
    assert a != b and (R.exact_d2(q, p) < a) != (R.exact_d2(q, p) < b)
    assert Fraction(float(R.r2_of(r))) == R.rnd32(Fraction(r) * Fraction(r))


def test_swap_pair_and_its_two_clouds():
    q, a, b = R.planted_swap()
    assert R.exact_d2(q, a) < R.exact_d2(q, b) and R.exact_d2(q, a, "fma_xy") > R.exact_d2(q, b, "fma_xy")
    for name, inside in (("knn_fma_swap_at_k", False), ("knn_fma_swap_inside", True)):
        c = R.search_case(name)
        ia, ib, k = _where(c, a), _where(c, b), c.note["k"]
        row = R.knn(c.x, c.ptr_x, c.q, c.ptr_q, k)[0][0].tolist()
        wrong = R.knn(c.x, c.ptr_x, c.q, c.ptr_q, k, form="fma_xy")[0][0].tolist()
        if inside:
            assert row.index(ia) + 1 == row.index(ib) < k - 1 and wrong.index(ib) + 1 == wrong.index(ia)
        else:
            assert row[k - 1] == ia and ib not in row and wrong[k - 1] == ib and ia not in wrong


def test_tie_case_has_the_lower_index_a_tile_and_a_run_later():
    c = R.search_case("knn_tie_lower_index_later")
    w = _w(c)
    first, second = int(np.flatnonzero(w == c.note["first"])[0]), int(np.flatnonzero(w == c.note["second"])[0])
    q = c.note["q"]
    assert R.exact_d2(q, c.x[first]) == R.exact_d2(q, c.x[second])
    assert first // R.TILE > second // R.TILE and c.keys[first] > c.keys[second] and w[first] < w[second]
    nbr, _ = R.knn(c.x, c.ptr_x, c.q, c.ptr_q, 4, R.X_INDEX_IN_W)
    assert nbr[0, 3] == w[first]
    assert R.knn(c.x, c.ptr_x, c.q, c.ptr_q, 4, 0)[0][0, 3] == second                      # by position the earlier one wins


def test_fourfold_duplicates_carry_descending_indices_inside_every_cell():
    c = R.search_case("knn_fourfold_duplicates_reversed")
    w, same = _w(c), c.keys[1:] == c.keys[:-1]
    assert same.sum() >= 270 and (np.diff(w)[same] < 0).all() and (np.diff(c.keys.astype(np.int64)) >= 0).all()
    assert all(((c.x[:, :3] == p).all(1)).sum() == 4 for p in c.x[::37, :3])


def test_tile_box_cases_sit_exactly_on_the_face():
    c = R.search_case("box_face_tie_needs_le")
    box = R.tile_bbox(c.x, c.ptr_x, 4)
    q, held, face = c.note["q"], c.note["held"], c.note["on_face"]
    assert R.box_gap2(box[0], q) == 0 and R.box_gap2(box[1], q) == R.d2_rows(q[None], c.x[face:face + 1])[0] == R.d2_rows(q[None], c.x[held:held + 1])[0]
    assert _w(c)[face] < _w(c)[held] and face // R.TILE == 1 and held // R.TILE == 0
    assert R.knn(c.x, c.ptr_x, c.q, c.ptr_q, 1, R.X_INDEX_IN_W)[0][0, 0] == _w(c)[face]
    gap2 = R.box_gap2(box[1], q)
    assert gap2 == R.r2_of(R.search_case("ball_box_gap_eq_r2").note["r"])
    assert gap2 == R.below(R.r2_of(R.search_case("ball_box_gap_below_r2").note["r"]))
    inside = R.ball(c.x, c.ptr_x, c.q, c.ptr_q, R.radius_above_quarter(), 64, 0)[0][0].tolist()
    assert face in inside and face not in R.ball(c.x, c.ptr_x, c.q, c.ptr_q, 0.25, 64, 0)[0][0].tolist()


def test_size_cases_hold_the_stated_counts():
    c = R.search_case("sizes_queries_per_voxel_B300")
    mq, nx = np.diff(c.ptr_q), np.diff(c.ptr_x)
    assert len(mq) == 300 and set(mq.tolist()) == {0, 1, 31, 32, 33, 63, 64, 65} and mq[0] == 0 and mq[-1] == 0 and (mq[7:10] == 0).all()
    assert nx[0] == 0 and nx[-1] == 0 and (nx[17:20] == 0).all() and nx[5] == 0 and mq[5] == 32   # queries without candidates
    want = {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1791, 1792, 1793, 3585}
    seen = set()
    for which in R.C_COUNTS:
        spread, one = R.search_case(f"sizes_cands_{which}_spread"), R.search_case(f"sizes_cands_{which}_one_cell")
        seen |= set(np.diff(spread.ptr_x).tolist())
        n = len(R.C_COUNTS[which])
        assert np.array_equal(np.diff(one.ptr_x)[:n], np.diff(spread.ptr_x))
        for b in range(n):                                                                   # one cell = one key per voxel
            assert len(np.unique(one.keys[one.ptr_x[b]:one.ptr_x[b + 1]])) == 1
        assert len(spread.x) <= 8192 and len(one.x) <= 8192
    assert seen == want
    c = R.search_case("sizes_k_and_cap_sweep")
    assert set(c.ks) == {1, 2, 7, 8, 63, 64, 65, 100} == {cap for _, cap in c.balls} and np.diff(c.ptr_x).min() == 5 < min(k for k in c.ks if k > 5)


def _grid(c):
    lo = c.grid[:12].view(F)
    return lo, float(c.grid[12:16].view(F)[0]), c.grid[32:56].view(np.int64)


@pytest.mark.parametrize("name,offset", [("grid_candidates_on_cell_faces", 0.0), ("grid_offset_plus_100", 100.0), ("grid_offset_minus_3", -3.0)])
def test_lattice_candidates_are_exactly_on_faces(name, offset):
    c = R.search_case(name)
    lo, res, dims = _grid(c)
    assert (lo == F(offset)).all() and res == 0.25 and dims.tolist() == [5, 5, 5]
    steps = (c.x[:, :3].astype(np.float64) - offset) / 0.25                                   # exact: multiples of 1/4 near 100 are float32
    on = (steps == np.round(steps)).all(1)
    assert on.sum() == c.note["lattice"] == 125
    assert np.array_equal(R.cells_of(c.x[on], lo, res), np.round(steps[on]).astype(np.int64))


def test_roundtrip_case_moves_the_nearest_neighbour_below_the_face_its_key_is_above():
    c = R.search_case("grid_roundtrip_moves_kth_across_face")
    lo, res, dims = _grid(c)
    w, q, face = _w(c), c.note["q"], F(c.note["face"])
    P, D = int(np.flatnonzero(w == c.note["P"])[0]), int(np.flatnonzero(w == c.note["D"])[0])
    row_of = lambda i: (int(c.keys[i]) // int(dims[0])) % int(dims[1])                       # noqa: E731
    assert (lo == 0).all() and row_of(P) == round(float(face) / res) and c.x[P, 1] == R.below(face)     # keyed above, lying below
    assert row_of(D) == row_of(P) - 1 == int((q[1] - lo[1]) / F(res))
    dP, dD = R.exact_d2(q, c.x[P]), R.exact_d2(q, c.x[D])
    gap = Fraction(float(face)) - Fraction(float(q[1]))
    assert dP < dD <= gap * gap and dD <= Fraction(float((face - q[1]) * (face - q[1])))
    assert R.knn(c.x, c.ptr_x, c.q, c.ptr_q, 1)[0][0, 0] == P
    assert (np.delete(R.d2(q[None], c.x)[0], [P, D]) > R.d2(q[None], c.x[D:D + 1])[0, 0]).all()


def _schedule(name):
    c = R.search_case(name)
    return c, R.slab_schedule(c, c.note["k"])


def test_growth_case_takes_exactly_one_more_pass():
    c, P = _schedule("grid_growth_one_more_pass")
    assert len(P) == 2 and not any(p["whole"] for p in P)
    assert P[0]["found"] == c.note["near"] < c.note["k"] and P[0]["left"] == 6 and P[1]["found"] >= c.note["k"] and P[1]["left"] == 0
    assert P[1]["box"][1] > P[0]["box"][1] and P[1]["box"][1] < _grid(c)[2][1] - 1              # grown, not yet at the grid face


def test_growth_case_ends_clamped_at_the_grid_face():
    c, P = _schedule("grid_growth_into_the_face_clamp")
    dims = _grid(c)[2]
    assert len(P) >= 3 and not any(p["whole"] for p in P) and [p["left"] for p in P[:-1]] == [6] * (len(P) - 1) and P[-1]["left"] == 0
    assert P[-2]["box"][1] < dims[1] - 1 and P[-1]["box"][:2] == (0, dims[1] - 1) and P[-1]["box"][2:] == (0, dims[2] - 1)
    assert P[-2]["found"] < c.note["k"] <= P[-1]["found"]


def test_give_up_case_reaches_pass_8_with_lists_to_forget():
    c, P = _schedule("grid_give_up_after_8_passes")
    assert len(P) == 9 and not any(p["whole"] for p in P[:8]) and P[8]["whole"] and P[8]["forgot"]
    assert all(c.note["near"] <= p["found"] < c.note["k"] and p["left"] == 6 for p in P[:8])   # partial lists, never k, nobody final
    assert all(p["box"][3] - p["box"][2] + 1 <= 128 for p in P[:8]) and P[8]["found"] == len(c.x) >= c.note["k"]
    assert all(b["rho"] > 2 * a["rho"] for a, b in zip(P[:8], P[1:]))                            # thr = +inf: the radius doubles


def test_fallback_case_exceeds_128_layers_after_partial_passes_and_forgets():
    c, P = _schedule("grid_fallback_over_128_layers_forgets")
    last = len(P) - 1
    assert 2 <= last < 8 and not any(p["whole"] for p in P[:last]) and P[last]["whole"] and P[last]["forgot"]
    assert all(p["box"][3] - p["box"][2] + 1 <= 128 and c.note["near"] <= p["found"] < c.note["k"] and p["left"] == 6 for p in P[:last])
    assert P[last]["box"][3] - P[last]["box"][2] + 1 > 128 and P[last]["found"] == len(c.x) >= c.note["k"]
    c, P = _schedule_k("grid_probe_region_over_128_layers", 2)
    assert len(P) == 1 and P[0]["whole"] and not P[0]["forgot"]                                 # the probe's own region: nothing to forget


def _schedule_k(name, k):
    c = R.search_case(name)
    return c, R.slab_schedule(c, k)


def test_grid_shape_cases():
    for a in range(3):
        assert _grid(R.search_case(f"grid_one_cell_thick_{'xyz'[a]}"))[2][a] == 1
    c = R.search_case("grid_box_more_than_256_runs")
    _, _, dims = _grid(c)
    assert len(np.unique(c.keys.astype(np.int64) // int(dims[0]))) == 400 and 2 * 400 > 256


def test_hint_cases():
    c = R.search_case("hints_planted")
    k1, k2, nine = c.note["k1"], c.note["k2"], c.note["nine"]
    assert nine == F(F(9) * F(0.25)) * F(0.25) and k2[0] == 0 and k1[0] == 0 and np.diff(c.ptr_x).tolist() == [300, 1]
    H = c.hints
    assert H["below_k2"][1][7] < k2[7] and H["below_k1"][1][7] < k1[7] and np.isinf(H["one_inf_k2"][1]).sum() == 1
    assert np.array_equal(np.delete(H["below_k2"][1], 7), np.delete(k2, 7)) and len(k2) > 32 and c.ptr_q[1] == 32
    assert H["hmax_9res2_k2"][1].max() == nine and H["hmax_above_9res2_k2"][1].max() == R.above(nine) and k2.max() < nine
    for k, h in (H[n] for n in H if not n.startswith("below")):                               # every other planted hint is a true upper bound
        assert (h >= (k1 if k == 1 else k2)).all()


@pytest.mark.parametrize("name", sorted(R.HINT2))
def test_hint2_is_never_below_the_second_nearest(name):
    q, rank, ptr_q, xc, ptr_c = R.hint2_case(name)[:5]
    h = R.knn_hint2(q, rank, ptr_q, xc)
    true2 = R.kth_d2(xc, ptr_c, q, ptr_q, 2)
    two = np.repeat(np.diff(ptr_c) >= 2, np.diff(ptr_q))
    assert (h[two] >= true2[two]).all() and np.isinf(h[~two]).all()
    if name == "hint2_single_cell":
        assert np.isinf(h).all() and ptr_c[-1] == 1
    if name.startswith("hint2_voxel_ends"):
        assert np.diff(ptr_q).tolist() == [1, 30, 50, 9, 40, 1] and np.diff(ptr_c)[[1, 3]].tolist() == [1, 1]


def test_sampler_cases():
    on_face, split = R.planted_cells()
    r = Fraction(float(F(0.04)))
    for p in on_face:                                                                        # float32 quotient exactly c, true quotient below c
        c = round(float(p) / 0.04)
        assert R.rnd32(Fraction(float(p)) / r) == c and Fraction(float(p)) / r < c
    for p in split:
        assert int(F(p) / F(0.04)) != int(F(p) * (F(1) / F(0.04))) and int(R.rnd32(Fraction(float(p)) / r)) == int(F(p) / F(0.04))
    assert len(on_face) >= 4 and len(split) >= 4
    S = R.sampled("sampler_extent_exact_multiple")
    top = (R.cells_of(R.sampler_case("sampler_extent_exact_multiple").xyzr, S.lo, 0.25) == 4).any(1)
    assert S.dims.tolist() == [5, 5, 5] and top.sum() == 1 and (S.hi - S.lo == 1).all()
    S = R.sampled("sampler_all_in_one_cell_n5000")
    assert S.idx.tolist() == [4999] and S.T == 1 and 5000 > 4096
    S = R.sampled("sampler_every_point_own_cell")
    assert len(S.idx) == 512 and np.array_equal(np.sort(S.idx), np.arange(512))
    assert [int(R.sampler_case(f"sampler_n_{n}").ptr[-1]) for n in (1, 4095, 4096, 4097, 8192)] == [1, 4095, 4096, 4097, 8192]
    S, c = R.sampled("sampler_empty_voxels_first_last_inside"), R.sampler_case("sampler_empty_voxels_first_last_inside")
    assert S.b_lo == 2 and c.ptr[-1] == c.ptr[-3] and (np.diff(S.ptr) > 0).tolist() == (np.diff(c.ptr) > 0).tolist()
    S = R.sampled("sampler_grid_over_2_32_cells")
    assert int(np.prod(S.dims.astype(object))) > 1 << 32 and int(S.cell_keys.max()) > 1 << 32 and S.T > 1 << 30
    S, c = R.sampled("sampler_table_cells_at_and_below_the_grid"), R.sampler_case("sampler_table_cells_at_and_below_the_grid")
    assert S.T == c.note["T"] and c.table_cells[:2] == (S.T, S.T - 1)
    assert all(len(R.sampler_case(n).xyzr) <= 8192 for n in R.SAMPLER)


def test_chain_input_has_points_the_round_trip_moves_across_faces():
    x, ptr, sf = R.chain_input()
    T = R.chain(x, ptr, sf)
    S = T["S"][0]
    crossed = (R.cells_of(x[S.idx], S.lo, R.CHAIN_RES[0]) != R.cells_of(T["xyzr"][1], S.lo, R.CHAIN_RES[0])).any(1)
    assert crossed[S.batch == 0].sum() >= 3 and crossed[S.batch == 1].sum() >= 3 and np.diff(ptr).tolist() == [600, 200]
    assert all(S_.T <= 1 << 14 for S_ in T["S"])


# ---- wrong kernels as variants of the reference ----------------------------------------------------------------------------------------

def _answers(c, knn_kw=None, ball_kw=None, r2=None):
    out = []
    for flags in (0, R.X_INDEX_IN_W):
        for k in c.ks:
            out.append(R.knn(c.x, c.ptr_x, c.q, c.ptr_q, k, flags, **(knn_kw or {})))
        for r, cap in c.balls:
            out.append(R.ball(c.x, c.ptr_x, c.q, c.ptr_q, r, cap, flags, r2=None if r2 is None else r2(r), **(ball_kw or {})))
    return out


def _changed(knn_kw=None, ball_kw=None, r2=None):
    names = set()
    for name in R.SEARCH:
        c = R.search_case(name)
        a, b = _answers(c), _answers(c, knn_kw, ball_kw, r2)
        if not all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b)):
            names.add(name)
    return names


def _group(*groups):
    return {n for n in R.SEARCH if R.search_case(n).group in groups}


EXACT_COORDINATES = {"box_face_tie_needs_le", "ball_box_gap_eq_r2", "ball_box_gap_below_r2"}

SEARCH_VARIANTS = {   # name: (keyword arguments of knn, of ball, r2, cases it must change, cases it must not change)
    "fma(dz,dz,fma(dy,dy,dx*dx))": (dict(form="fma_xy"), dict(form="fma_xy"), None,
                                     {"ball_sum_in_fma_out", "ball_sum_out_fma_in", "knn_fma_swap_at_k", "knn_fma_swap_inside"}, {"ball_d2_eq_r2"}),
    "fma(dz,dz,dx*dx+dy*dy)": (dict(form="fma_z"), dict(form="fma_z"), None, {"ball_sum_in_fmaz_out", "ball_sum_out_fmaz_in"}, {"ball_d2_eq_r2"}),
    "dx*dx+(dy*dy+dz*dz)": (dict(form="reassoc"), dict(form="reassoc"), None, {"ball_sum_in_reassoc_out", "ball_sum_out_reassoc_in"}, {"ball_d2_eq_r2"}),
    "float64 predicate": (None, dict(form="f64"), None, {"ball_f32_in_f64_out", "ball_f32_out_f64_in"}, {"ball_d2_below_r2", "ball_d2_above_r2"}),
    "<= for <": (None, dict(strict=False), None, {"ball_d2_eq_r2", "ball_box_gap_eq_r2"},
                 {"ball_d2_below_r2", "ball_d2_above_r2", "ball_box_gap_below_r2"} | _group("knn_order", "sizes", "grid", "hints")),
    "float32(r) squared": (None, None, R.r2_f32, {"ball_radius_f32_squared"}, {"ball_" + p for p in PAIRS} | _group("knn_order", "sizes", "grid", "hints")),
    "ties by storage position": (dict(tie="storage"), None, None, {"knn_tie_lower_index_later", "knn_fourfold_duplicates_reversed", "box_face_tie_needs_le"},
                                 _group("predicate", "sizes", "hints")),
    "first cap in storage order": (None, dict(first="storage"), None, {"knn_fourfold_duplicates_reversed", "sizes_k_and_cap_sweep", "ball_d2_eq_r2"},
                                   EXACT_COORDINATES | _group("hints")),
}


@pytest.mark.parametrize("variant", sorted(SEARCH_VARIANTS))
def test_search_variant_changes_its_stated_cases_and_no_spared_one(variant):
    knn_kw, ball_kw, r2, kills, spares = SEARCH_VARIANTS[variant]
    changed = _changed(knn_kw, ball_kw, r2)
    assert kills <= changed, sorted(kills - changed)
    assert not (spares & changed), sorted(spares & changed)
    if "fma" in variant or "+(" in variant:                                # arithmetic forms agree wherever the arithmetic is exact
        assert not (EXACT_COORDINATES & changed)


def _sampler_changed(**kw):
    names = set()
    for name in R.SAMPLER:
        c, a = R.sampler_case(name), R.sampled(name)
        b = R.sample(c.xyzr, c.ptr, c.res, **kw)
        if not all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("idx", "ptr", "batch", "inv", "sorted_keys", "cell_keys", "rank_sorted", "grid")):
            names.add(name)
    return names


SAMPLER_VARIANTS = {
    "reciprocal multiply": (dict(cells="mul"), {"sampler_div_and_mul_cells_differ"}, {"sampler_all_in_one_cell_n5000", "sampler_n_1", "sampler_every_point_own_cell"}),
    "float64 cells": (dict(cells="f64"), {"sampler_points_on_faces_quotient_exact"}, {"sampler_all_in_one_cell_n5000", "sampler_n_1"}),
    "dims without the + 1": (dict(plus1=False), {"sampler_extent_exact_multiple", "sampler_n_1"}, set()),
    "smallest index as representative": (dict(rep="min"), {"sampler_all_in_one_cell_n5000", "sampler_n_8192", "sampler_extent_exact_multiple"},
                                         {"sampler_every_point_own_cell", "sampler_n_1", "sampler_grid_over_2_32_cells"}),
}


@pytest.mark.parametrize("variant", sorted(SAMPLER_VARIANTS))
def test_sampler_variant_changes_its_stated_cases_and_no_spared_one(variant):
    kw, kills, spares = SAMPLER_VARIANTS[variant]
    changed = _sampler_changed(**kw)
    assert kills <= changed, sorted(kills - changed)
    assert not (spares & changed), sorted(spares & changed)


@pytest.mark.parametrize("variant,kw,kills,spares", [
    ("window across voxels", dict(cross=True), {"hint2_voxel_ends_own_order", "hint2_voxel_ends_sorted_order"}, {"hint2_one_point", "hint2_single_cell"}),
    ("hint = d1 alone", dict(d1_only=True), set(R.HINT2), set()),
])
def test_hint2_variant_changes_its_stated_cases_and_no_spared_one(variant, kw, kills, spares):
    changed = set()
    for name in R.HINT2:
        q, rank, ptr_q, xc, _ = R.hint2_case(name)[:5]
        if not np.array_equal(R.bits(R.knn_hint2(q, rank, ptr_q, xc)), R.bits(R.knn_hint2(q, rank, ptr_q, xc, **kw))):
            changed.add(name)
    assert kills <= changed and not (spares & changed), (sorted(kills - changed), sorted(spares & changed))
    if "window" in variant:                                                # the one-point voxels at both ends see their neighbours' ranks
        q, rank, ptr_q, xc, _ = R.hint2_case("hint2_voxel_ends_own_order")[:5]
        wrong = R.knn_hint2(q, rank, ptr_q, xc, cross=True)
        assert np.isinf(R.knn_hint2(q, rank, ptr_q, xc)[[0, -1]]).all() and np.isfinite(wrong[[0, -1]]).all()
