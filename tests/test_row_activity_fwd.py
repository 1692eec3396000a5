"""Row activity of the sparse regression FORWARD, CPU tier: the numpy references in ``ops/halo.py`` that the device
kernels (csrc/kernels/row_activity.hip) are tested against -- the positive-row mask from the anchor states, the
un-extended tile rule against a brute-force loop over the boxes, and the identity that lets the forward reuse the
backward's lists: the un-extended list of ``M_k`` is the extended list of ``M_{k-1}``."""
import numpy as np

from batchai_retinanet_horovod_coco_amd.ops import halo

GEOMS = {
    # width 100: column-split boxes (COLMAX 84)
    "wide": (2, ((20, 100), (10, 50), (5, 25), (3, 13), (2, 7))),
    # 382 rows per image, no multiple of 64: K-tiles straddle levels and images
    "ragged": (3, ((13, 21), (7, 11), (4, 6), (2, 3), (1, 2))),
}
GROUP = 9


def _rows(N, shapes):
    return N * sum(h * w for h, w in shapes)


def test_rows_positive_reference():
    rng = np.random.default_rng(0)
    for N, shapes in GEOMS.values():
        M = _rows(N, shapes)
        # -1 ignore, 0 negative, 1 positive: only the 1s count
        state = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=M * GROUP, p=(0.1, 0.88, 0.02))
        state[:GROUP] = 0
        state[GROUP - 1] = 1                      # the last anchor of row 0
        state[GROUP:2 * GROUP] = -1               # a row of ignored anchors is not positive
        state[(M - 1) * GROUP] = 1                # the first anchor of the last row
        got = halo.rows_positive(state, GROUP)
        assert got.dtype == bool and got.shape == (M,)
        assert np.array_equal(got, (state.reshape(M, GROUP) == 1).any(1))
        assert got[0] and not got[1] and got[M - 1]
        # group 1: the state itself
        assert np.array_equal(halo.rows_positive(state[:M], 1), state[:M] == 1)
        words = halo.pack_row_bits(got)
        if M % 64:
            assert int(words[-1]) >> (M % 64) == 0


def _brute_unextended(tab, rows):
    """A tile is active when one of its own output pixels is set: pixel by pixel over every box."""
    act = np.zeros(len(tab), dtype=bool)
    for i, row in enumerate(tab):
        for (sbeg, hoff, ib, ob, H, W, y0, x0, R, C) in halo._boxes(row):
            for r in range(R):
                for c in range(C):
                    if rows[ob + (y0 + r) * W + x0 + c]:
                        act[i] = True
    return act


def test_unextended_rule_against_brute_force():
    rng = np.random.default_rng(1)
    for N, shapes in GEOMS.values():
        M = _rows(N, shapes)
        tab = halo.build_tiles(N, shapes)
        for frac in (0.0, 0.003, 0.02, 1.0):
            rows = rng.random(M) < frac
            if 0 < frac < 1:
                rows[0] = rows[M - 1] = True
            act = halo.active_tiles(tab, rows, ext=0)
            assert np.array_equal(act, _brute_unextended(tab, rows)), frac
            # every pixel belongs to one tile: the active tiles' rows are a superset of the mask, and tight
            assert not (rows & ~halo.tile_rows(tab, act, M)).any()
            assert act.any() == bool(rows.any()) and (frac < 1 or act.all())
            # the extended rule (the default) is the wider one
            assert not (act & ~halo.active_tiles(tab, rows)).any()
            assert np.array_equal(halo.active_tiles(tab, rows), halo.active_tiles(tab, rows, ext=1))


def test_unextended_list_of_mk_is_extended_list_of_mk_minus_1():
    rng = np.random.default_rng(2)
    for N, shapes in GEOMS.values():
        M = _rows(N, shapes)
        tab = halo.build_tiles(N, shapes)
        for frac in (0.002, 0.01):
            cur = rng.random(M) < frac
            cur[0] = cur[M - 1] = cur[M // 2] = True
            for k in range(1, 5):
                nxt = halo.dilate_rows(cur, N, shapes)
                assert np.array_equal(halo.active_tiles(tab, nxt, ext=0), halo.active_tiles(tab, cur, ext=1)), (frac, k)
                cur = nxt
