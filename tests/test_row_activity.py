"""Row activity of the sparse regression gradient, CPU tier: the numpy references in ``ops/halo.py`` that the device
kernels (csrc/kernels/row_activity.hip) are tested against -- the tile-activity rule against the true support of the
halo kernel model, the dilation against a brute force, and the packed-row bit layout."""
import numpy as np

from batchai_retinanet_horovod_coco_amd.ops import halo

SHAPES_A = ((6, 100), (3, 50), (2, 7))                      # width 100: column-split boxes (COLMAX 84)
SHAPES_B = ((13, 21), (7, 11), (4, 6), (2, 3), (1, 2))      # 382 rows per image: K-tiles straddle levels and images


def _decode(m, N, shapes):
    img = sum(h * w for h, w in shapes)
    b, q = divmod(m, img)
    for lv, (h, w) in enumerate(shapes):
        if q < h * w:
            return b, lv, q // w, q % w
        q -= h * w
    raise AssertionError(m)


def _base(b, lv, shapes):
    img = sum(h * w for h, w in shapes)
    return b * img + sum(h * w for h, w in shapes[:lv])


def test_active_tiles_cover_the_true_support():
    rng = np.random.default_rng(0)
    for N, shapes in ((1, SHAPES_A), (2, SHAPES_B)):
        tab = halo.build_tiles(N, shapes)
        halo.check_tiles(tab, N, shapes)
        P = N * sum(h * w for h, w in shapes)
        for frac in (0.0, 0.01, 0.05):
            rows = rng.random(P) < frac
            if frac:
                rows[0] = rows[P - 1] = True
            # positive inputs and weights: no cancellation, the output support is the exact 3x3 dilation
            x = rng.random((P, 2)) * rows[:, None]
            w = rng.random((3, 3, 3, 2)) + 0.1
            y = halo.emulate(x, w, tab)
            support = (y != 0).any(axis=1)
            assert np.array_equal(support, halo.dilate_rows(rows, N, shapes))
            act = halo.active_tiles(tab, rows)
            covered = halo.tile_rows(tab, act, P)
            assert not (support & ~covered).any()
            # and the rule is tight: every active tile holds a non-zero output
            for i in np.nonzero(act)[0]:
                only = np.zeros(len(tab), dtype=bool)
                only[i] = True
                assert (support & halo.tile_rows(tab, only, P)).any(), i
            assert act.any() == bool(rows.any())


def test_dilation_matches_brute_force_and_bit_layout():
    rng = np.random.default_rng(1)
    for N, shapes in ((2, SHAPES_A), (3, SHAPES_B)):
        P = N * sum(h * w for h, w in shapes)
        rows = rng.random(P) < 0.02
        rows[0] = rows[P - 1] = True
        brute = np.zeros(P, dtype=bool)
        for m in np.nonzero(rows)[0]:
            b, lv, y, x = _decode(int(m), N, shapes)
            H, W = shapes[lv]
            for yy in range(max(0, y - 1), min(H, y + 2)):
                for xx in range(max(0, x - 1), min(W, x + 2)):
                    brute[_base(b, lv, shapes) + yy * W + xx] = True
        assert np.array_equal(halo.dilate_rows(rows, N, shapes), brute)
        words = halo.pack_row_bits(brute)
        assert words.dtype == np.uint64 and words.shape == ((P + 63) // 64,)
        for m in range(P):
            assert bool((int(words[m // 64]) >> (m % 64)) & 1) == bool(brute[m])
        if P % 64:
            assert int(words[-1]) >> (P % 64) == 0           # nothing past the last row
        assert np.array_equal(halo.unpack_row_bits(words, P), brute)
        # word t is K-tile t: it is zero exactly when none of its 64 rows is set
        pad = np.zeros(len(words) * 64, dtype=bool)
        pad[:P] = brute
        assert np.array_equal(words != 0, pad.reshape(-1, 64).any(axis=1))
