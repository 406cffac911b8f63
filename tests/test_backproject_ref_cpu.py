"""tests/backproject_ref.py held to the project's pinned oracles (oracle/backproject.py, itself pinned to the reference's
PointCloudClassifier by tests/test_host_golden.py, and scipy's KD-tree), and the inputs of tests/test_gpu_backproject_kernels.py held
to the conditions they are named for.  No GPU: the conditions are statements about the inputs, checked on the reference alone."""
import numpy as np
import pytest

from oracle import backproject as OB
from tests import backproject_ref as R


# ---- the restatement against the oracles ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,any_wood", [(64, 1.0), (32, 0.5), (32, 0.9)])
def test_vote_at_full_rows_is_compute_labels(k, any_wood):
    g = np.random.default_rng(3)
    nc, n = 2000, 600
    prob = g.random(nc).astype(np.float32)
    prob[g.integers(0, nc, 300)] = 0.5
    # (predictions of prob >= 0.5 would let wood win every vote, wood in every second point would meet every any-wood row)
    pred = (g.random(nc) < (0.5 if any_wood == 1 else 0.02)).astype(np.float32)
    nbr = g.integers(0, nc, (n, k)).astype(np.int32)
    cls = np.zeros((nc, 5))
    cls[:, 3], cls[:, 4] = pred, prob
    want = OB.compute_labels(cls[nbr], any_wood)
    label, pwood, undecided = R.vote(nbr, np.full(n, k), k, pred, prob, any_wood)
    assert not undecided.any()
    assert np.array_equal(label, want[:, 0].astype(np.float32))
    assert np.array_equal(pwood, want[:, 1].astype(np.float32))
    assert 0.05 < label.mean() < 0.99                                      # both labels occur


def test_vote_takes_the_first_deg_slots_and_nothing_else():
    """compute_labels on the truncated row = vote with that deg; deg above k counts as k; an empty row gives (0, 0).  A row of ONE
    slot: compute_labels counts as many classes as the row is long (predicter.py:115-116, sic), so it can only answer 0 there; the
    header's rule is the argmax over {0, 1}, which a single wood neighbour of positive probability wins."""
    pred, prob = R.vote_table()
    cls = np.zeros((R.VOTE_NC, 5))
    cls[:, 3], cls[:, 4] = pred, prob
    for k in (5, 64):
        nbr, deg = R.vote_case(40, k)
        for any_wood in (1.0, 0.5):
            label, pwood, _ = R.vote(nbr, deg, k, pred, prob, any_wood)
            for i in range(40):
                c = min(int(deg[i]), k)
                want = OB.compute_labels(cls[nbr[i:i + 1, :c]], any_wood)[0] if c else (0.0, 0.0)
                if c == 1 and any_wood == 1:
                    assert want[0] == 0
                    want = (float(pred[nbr[i, 0]] == 1 and prob[nbr[i, 0]] > 0), want[1])
                assert (label[i], pwood[i]) == (np.float32(want[0]), np.float32(want[1])), (k, any_wood, i)


def test_refine_is_the_kd_tree_where_the_order_is_unique():
    from scipy.spatial import cKDTree
    cand, q, d2, full = R.uniform_ranked()
    for k in (1, 32, 64):
        d, idx = cKDTree(cand).query(q, k=k + 1)
        strict = (np.diff(d, axis=1) > 0).all(1)
        assert strict.mean() > 0.99
        got = R.refine(cand, q, k)
        assert got.shape == (R.M, k)
        assert np.array_equal(got[strict], idx[strict, :k])
    assert np.array_equal(R.refine(cand[:20], q, 64), full_of(cand[:20], q))   # nc < k: all of them


def full_of(cand, q):
    return R.ranking(cand, q)[1]


def test_refine_orders_equal_distances_by_index():
    cand = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    assert R.refine(cand, np.zeros((1, 3)), 3).tolist() == [[2, 0, 1]]
    assert R.refine(cand[::-1], np.zeros((1, 3)), 5).tolist() == [[2, 0, 1, 3, 4]]


MORTON_TABLE = [   # lo = (0, 0, 0), res = 1: (x, y, z), key
    ((0.0, 0.0, 0.0), 0), ((1.5, 0.0, 0.0), 1), ((0.0, 1.0, 0.0), 2), ((0.0, 0.0, 1.99), 4), ((1.0, 1.0, 1.0), 7),
    ((2.0, 0.0, 0.0), 8), ((3.0, 3.0, 3.0), 63), ((5.0, 0.0, 2.0), 97),
    ((2097151.0, 0.0, 0.0), 0x1249249249249249),                      # the last cell: 21 ones, every third bit
    ((0.0, 2097151.0, 0.0), 0x2492492492492492), ((0.0, 0.0, 2097151.0), 0x4924924924924924),
    ((-0.5, 1.0, 0.0), 2),                                            # below lo -> cell 0
    ((-1e30, -np.inf, 1.0), 4),
    ((1e9, 0.0, 0.0), 0x1249249249249249),                            # beyond 2^21 cells -> the last cell
    ((np.inf, 1e38, 4e6), 0x7fffffffffffffff),
    ((np.nan, 1.0, 0.0), 2), ((np.nan, np.nan, np.nan), 0),          # NaN -> cell 0
    ((1.25, 0.0, 0.0), 1), ((0.0, 0.0, 0.0), 0), ((1.75, 0.5, 0.5), 1),
]


def test_morton_on_a_hand_written_table():
    xyz = np.array([p for p, _ in MORTON_TABLE], dtype=np.float32)
    keys, order = R.morton(xyz, (0.0, 0.0, 0.0), 1.0)
    # x = 5 = 0b101 -> bits 0 and 6; z = 2 = 0b10 -> bit 3 * 1 + 2 = 5
    assert MORTON_TABLE[7][1] == (1 << 0) | (1 << 6) | (1 << 5)
    assert keys.tolist() == [key for _, key in MORTON_TABLE]
    assert sorted(order.tolist()) == list(range(len(xyz)))
    assert (np.diff(keys[order].astype(np.float64)) >= 0).all()
    for key in (0, 1, 2):                                             # equal keys stay in input order
        same = [i for i, (_, v) in enumerate(MORTON_TABLE) if v == key]
        assert len(same) >= 2 and [i for i in order.tolist() if i in same] == same
    # float32 arithmetic with an origin and a cell size: (0.5f - 0.1f) / 0.1f rounds to 4.0 in float32 -> cell 4 = 0b100 -> bit 6;
    # the same float32 values divided in float64 give 3.99999994
    f = np.float32
    keys, _ = R.morton(np.array([[0.5, 1.0, 1.0]], dtype=f), (0.1, 1.0, 1.0), 0.1)
    assert keys.tolist() == [64]
    assert int(np.floor((float(f(0.5)) - float(f(0.1))) / float(f(0.1)))) == 3


# ---- the GPU cases meet their conditions ------------------------------------------------------------------------------------------------

def test_uniform_queries_are_where_the_case_says():
    for shifted in (False, True):
        cand, q, d2, full = R.uniform_ranked(shifted)
        s = np.asarray(R.SURVEY_OFFSET if shifted else (0.0, 0.0, 0.0))
        assert cand.shape == (R.NC, 3) and q.shape == (R.M, 3) and R.M % 4 == 3 and R.NC > 256
        lo, hi = cand.min(0), cand.max(0)
        below, above = q < lo, q > hi
        assert (~(below | above).any(1)).sum() >= 80
        sides = {tuple(r) for r in (above.astype(int) - below.astype(int))[80:132]}
        assert len(sides) == 26                                       # every face, edge and corner of the box
        off = np.where(below, lo - q, np.where(above, q - hi, 0.0))
        assert off.max() <= 1.0 + 1e-9 and (np.abs(off[80:132].max(1) - 1.0) < 1e-9).sum() >= 26
        if not shifted:
            on = ((q[132:] - lo) / R.CELL32)
            assert (np.abs(on - np.round(on)) < 1e-9).any(1).all() and (np.abs(on - np.round(on)) < 1e-9).all(1).sum() >= 10
        assert np.array_equal(cand, R.uniform_cloud()[0] + s)


@pytest.mark.parametrize("shifted", [False, True])
def test_refine_targets_reach_their_T(shifted):
    cand, q, d2, full = R.uniform_ranked(shifted)
    assert (np.diff(np.take_along_axis(d2, full, 1), axis=1) > 0).all()    # no two candidates of a query tie: T = t exactly
    for k, t in R.REFINE_TARGETS:
        rows = R.rows_for_target(full, k, t, seed=t)
        assert rows.shape == (R.M, k) and all(len(set(r)) == k for r in rows.tolist())
        assert (rows == full[:, t - 1:t]).sum(1).tolist() == [1] * R.M
        assert (R.within(cand, q, rows) == t).all()
        if t > k:
            assert (np.sort(rows, 1) != np.sort(full[:, :k], 1)).any(1).mean() > 0.9   # the answer was not handed in
    assert {t <= 128 for _, t in R.REFINE_TARGETS} == {True, False}
    assert {127, 128, 129, R.NC} <= {t for _, t in R.REFINE_TARGETS}
    far = R.farthest_rows(full, 64, seed=5)
    assert (R.within(cand, q, far) == R.NC).all() and np.array_equal(np.sort(far, 1), np.sort(full[:, -64:], 1))


def test_tie_cases_tie_where_they_say():
    cand, members = R.tie_cloud()
    assert [len(members[n]) for n in ("star_odd", "star_even", "pile128", "pile129")] == [140, 141, 128, 129]
    for name, idx in members.items():                                 # planted at scattered indices, not a block
        assert idx.max() - idx.min() > 10 * len(idx) // 9
    for k in R.TIE_KS:
        q, rows, T = R.tie_case(k)
        assert np.array_equal(R.within(cand, q, rows), T)
        assert T[0] == k + 1 <= 128 and T[1] > 128 and T[2] == 128 and T[3] == 129
        d2, full = R.ranking(cand, q)
        star = "star_odd" if k % 2 else "star_even"
        for r in (0, 1):
            assert set(full[r, :T[1]].tolist()) == set(members[star].tolist())
            assert d2[r, full[r, k - 1]] == d2[r, full[r, k]] and full[r, k - 1] < full[r, k]      # bit-equal across the k-th place
            assert d2[r, full[r, k]] < d2[r, full[r, k + 1]] and (k == 1 or d2[r, full[r, k - 2]] < d2[r, full[r, k - 1]])
            assert cand[full[r, k - 1]].tolist() != cand[full[r, k]].tolist()                       # two distinct points
        assert full[0, k - 1] not in rows[0] and full[0, k] in rows[0]                               # handed the loser
        for r, pile in ((2, "pile128"), (3, "pile129"), (4, "pile129"), (5, "pile128")):
            assert np.array_equal(full[r, :k], members[pile][:k]) and len(np.unique(d2[r, members[pile]])) == 1
            assert set(rows[r].tolist()) <= set(members[pile].tolist())
        assert not set(rows[2].tolist()) & set(full[2, :k].tolist()) or k > 64
        assert rows[4].tolist() == full[4, :k][::-1].tolist()


def test_few_clouds_hold_fewer_than_k():
    for nc in (1, 20):
        cand, q, rows, deg = R.few_cloud(nc)
        assert len(cand) == nc < 64 and (deg == nc).all() and (rows[:, nc:] == R.SENTINEL).all()
        assert np.array_equal(np.sort(rows[:, :nc], 1), np.broadcast_to(np.arange(nc), (len(q), nc)))
        assert ((q < cand.min(0)) | (q > cand.max(0))).any(1).sum() >= 10
        if nc > 1:
            assert (rows[:, :nc] != R.refine(cand, q, 64)).any(1).mean() > 0.9                      # not handed in order


def test_vote_cases_cover_every_count_and_are_decided():
    pred, prob = R.vote_table()
    assert len(np.unique(prob)) < 0.7 * R.VOTE_NC and set(np.unique(pred)) == {0.0, 1.0}
    seen = set()
    for k in R.VOTE_KS:
        for n in R.VOTE_NS:
            for variant in range(5 if n < 5 else 1):
                nbr, deg = R.vote_case(n, k, variant)
                assert nbr.shape == (n, k) and deg.min() >= 0
                valid = np.arange(k)[None, :] < np.minimum(deg, k)[:, None]
                assert ((nbr[valid] >= 0) & (nbr[valid] < R.VOTE_NC)).all()
                assert np.isin(nbr[~valid], R.GARBAGE).all()
                seen |= {(k, int(d)) for d in deg}
                for any_wood in R.VOTE_ANY_WOOD:
                    label, pwood, undecided = R.vote(nbr, deg, k, *R.vote_table(rare=any_wood != 1), any_wood)
                    assert not undecided.any()
                    if n == 257:
                        assert 2 <= label.sum() <= n - 2              # both labels occur
        assert {(k, d) for d in range(k + 1)} | {(k, k + 5)} <= seen    # 0, 1, odd, even, k and one above k
        # the same counts at n = 1, where the only row is the last of its workgroup
        assert {int(R.vote_case(1, k, v)[1][0]) for v in range(5)} == {0, 1, k - 1, k, k + 5}


@pytest.mark.parametrize("k", R.VOTE_PLANTED_KS)
def test_planted_vote_rows_are_what_they_claim(k):
    (nbr, deg, pred, prob, aw, want), (nbr2, deg2, pred2, prob2, aw2, want2) = R.vote_planted(k)
    assert aw == 1.0 and aw2 == 0.5
    assert np.array_equal(prob * 1024, np.round(prob * 1024))
    label, _, undecided = R.vote(nbr, deg, k, pred, prob, aw)
    assert not undecided.any() and np.array_equal(label, want) and want.tolist() == [0, 1, 0, 0, 0]
    e = 2.0 ** -10
    sums = []
    for i in range(3):
        j = nbr[i, :deg[i]]
        sums.append(float(prob[j][pred[j] == 1].astype(np.float64).sum() - prob[j][pred[j] == 0].astype(np.float64).sum()))
    assert sums == [0.0, e, -e]
    label2, _, _ = R.vote(nbr2, deg2, k, pred2, prob2, aw2)
    assert np.array_equal(label2, want2) and want2.tolist() == [1, 1, 0, 0]
    wood = pred2[np.clip(nbr2, 0, len(pred2) - 1)] == 1
    assert wood.sum(1).tolist() == [1, 1, 1, 1]                                  # one wood neighbour per row ...
    assert np.argmax(wood, 1).tolist() == [k - 1, deg2[1] - 1, deg2[2], deg2[3]]  # ... last valid slot twice, slot deg twice


def test_morton_records_hold_what_they_say():
    lo = np.asarray(R.MORTON_LO, dtype=np.float32)
    key_bytes = {}
    for res in R.MORTON_RES:
        for beyond in (False, True):
            for n in R.MORTON_NS:
                rec = R.morton_records(n, beyond)
                assert rec.shape == (n, 4) and rec.dtype == np.float32
                keys, order = R.morton(rec[:, :3], lo, res)
                assert sorted(order.tolist()) == list(range(n))
                if n >= 255:
                    x = rec[:, :3]
                    cells = R.morton_cells(x, lo, res)
                    assert np.isnan(x).any(1).sum() >= 6 and (x < lo).any(1).sum() >= 6
                    with np.errstate(all="ignore"):
                        raw = np.floor((x.astype(np.float64) - lo) / np.float32(res))
                    if beyond:
                        assert (raw > 2 ** 21 - 1).any(1).sum() >= 9 and (cells == 2 ** 21 - 1).any(1).sum() >= 9
                    assert np.unique(keys, return_counts=True)[1].max() >= min(300, n // 3)       # a long run of one key
                    assert len(np.unique(keys)) > 30
            key_bytes[res, beyond] = (int(keys.max()).bit_length() + 7) // 8
    # bytes of the widest key = the radix sort's passes: they follow the cell size (the farthest ordinary record, z = 7, lies 40 /
    # 1024 / 2^22 cells above lo: 6 / 11 / 21 bits per axis), and a clamped record needs all eight
    assert [key_bytes[res, False] for res in R.MORTON_RES] == [3, 5, 8]
    assert [key_bytes[res, True] for res in R.MORTON_RES] == [8, 8, 8]
    # the finest grid spreads the ordinary records over all 21 bits of every axis
    fine = R.morton_cells(R.morton_records(4097)[:, :3], lo, R.MORTON_RES[2])
    ordinary = fine[(fine < 2 ** 21 - 1).all(1)]
    assert all(int(np.bitwise_or.reduce(ordinary[:, a])) == 2 ** 21 - 1 for a in range(3))
