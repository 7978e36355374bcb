"""Tiled pages (DESIGN.md "Tiled pages") restated in numpy: the tile plan (integers) and the stitch (float32, every operation rounded on its own).
Written from the rule's text, not from the C++: tests hold ttr_tile_plan / ttr_stitch_tiles / tile_stitch_kernel to it bit for bit."""
import numpy as np


def c32(x: int) -> int:
    return -(-x // 32) * 32


def axis(L: int, S: int, O: int):
    """one axis of length L -> (origins, extents, tile canvas)"""
    if L <= S:
        return [0], [L], c32(L)
    D = S - O
    n = -(-(L - S) // D) + 1
    o = [k * D for k in range(n - 1)] + [c32(L - S)]
    return o, [min(S, L - ok) for ok in o], S


def plan(h: int, w: int, S: int, O: int):
    oy, ey, Hc = axis(h, S, O)
    ox, ex, Wc = axis(w, S, O)
    return dict(ny=len(oy), nx=len(ox), oy=oy, ox=ox, ey=ey, ex=ex, Hc=Hc, Wc=Wc, H2=c32(h) // 2, W2=c32(w) // 2)


def seams(o, s):
    """heat-map seam centres of origins o (image pixels) for tile maps of length s"""
    return [(o[k + 1] // 2 + o[k] // 2 + s) // 2 for k in range(len(o) - 1)]


def axis_invariants(L: int, S: int, O: int):
    """the properties section 1 of the rule promises, for one axis; raises AssertionError naming the one that fails"""
    o, e, canvas = axis(L, S, O)
    n = len(o)
    assert all(v % 32 == 0 for v in o), ("origins are multiples of 32", L, S, O, o)
    assert all(o[k] < o[k + 1] for k in range(n - 1)), ("origins ascend", L, S, O, o)
    assert o[-1] + canvas == c32(L), ("the last tile ends at c32(L)", L, S, O, o)
    assert all(0 < e[k] <= canvas for k in range(n)), ("extents", L, S, O, e)
    assert o[-1] + e[-1] == L and all(o[k] + e[k] <= L for k in range(n)), ("tiles stay on the page", L, S, O)
    assert all(c32(e[k]) == canvas for k in range(n)), ("every tile alone, as an image of its extent, has the shared canvas", L, S, O, e)
    assert all(o[k] + canvas - o[k + 1] >= O for k in range(n - 1)), ("every overlap is at least O", L, S, O, o)
    s, c = canvas // 2, seams(o, canvas // 2)
    for k, ck in enumerate(c):
        assert ck % 8 == 0, ("seams are multiples of 8", L, S, O, c)
        assert o[k + 1] // 2 <= ck - 8 and ck + 8 <= o[k] // 2 + s, ("a band lies inside its overlap", L, S, O, k)
        if k:
            assert c[k - 1] + 8 <= ck - 8, ("bands do not touch", L, S, O, c)
    return n


def _segments(o, s, M):
    """per map coordinate u: (tile k, blend flag, weight of tile k + 1 as float32)"""
    k_of, blend, t = np.zeros(M, np.int64), np.zeros(M, bool), np.zeros(M, np.float32)
    c = seams(o, s)
    for u in range(M):
        k = len(o) - 1
        for i, ci in enumerate(c):
            if u < ci - 8:
                k = i
                break
            if u < ci + 8:
                k, blend[u] = i, True
                t[u] = np.float32(2 * (u - (ci - 8)) + 1) / np.float32(32)
                break
        k_of[u] = k
    return k_of, blend, t


def _lerp(a, b, t):
    """a + t (b - a) on float32 arrays, three roundings"""
    with np.errstate(all="ignore"):
        d = (b - a).astype(np.float32)
        m = (t * d).astype(np.float32)
        return (a + m).astype(np.float32)


def stitch(tiles, oy, ox, Hc, Wc, H2, W2):
    """tiles f32 [ny * nx, Hc / 2, Wc / 2, 2] of ONE page in (ty, tx) order -> f32 [H2, W2, 2]: x first, then y"""
    tiles = np.asarray(tiles, np.float32)
    ny, nx, sy, sx = len(oy), len(ox), Hc // 2, Wc // 2
    assert tiles.shape == (ny * nx, sy, sx, 2), tiles.shape
    kx, bx, tx = _segments(ox, sx, W2)
    ky, by, ty = _segments(oy, sy, H2)
    xs = np.arange(W2)
    rows = []                                   # per tile row: [sy, W2, 2], blended along x
    for r in range(ny):
        lx = xs - np.asarray(ox)[kx] // 2
        a = tiles[r * nx + kx, :, lx, :]        # [W2, sy, 2]
        k1 = np.minimum(kx + 1, nx - 1)
        lx1 = np.clip(xs - np.asarray(ox)[k1] // 2, 0, sx - 1)
        b = tiles[r * nx + k1, :, lx1, :]
        v = np.where(bx[:, None, None], _lerp(a, b, tx[:, None, None]), a)
        rows.append(np.ascontiguousarray(v.transpose(1, 0, 2)))
    out = np.zeros((H2, W2, 2), np.float32)
    for y in range(H2):
        k = int(ky[y])
        a = rows[k][y - oy[k] // 2]
        if by[y]:
            b = rows[k + 1][y - oy[k + 1] // 2]
            out[y] = _lerp(a, b, ty[y])
        else:
            out[y] = a
    return out


def seeded_tiles(seed, ntiles, sy, sx, pages=1):
    """heat-like maps with the awkward values in: negative zeros, denormals of both signs, values near FLT_MAX, and NaN in one tile (the last of page 0).
    The huge values are positive, in [3.0e38, 3.3e38]: the rule a + t (b - a) overflows once |b - a| passes FLT_MAX, and inf - inf in the second blend would
    GENERATE a NaN, whose sign bit is the platform's own (the rule says nothing about it); a NaN that is an INPUT, as in the one tile, is propagated."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((pages * ntiles, sy, sx, 2)).astype(np.float32)
    flat = t.reshape(-1)
    idx = rng.permutation(flat.size)
    q = flat.size // 50
    flat[idx[:q]] = np.float32(-0.0)
    flat[idx[q:2 * q]] = (rng.integers(1, 1 << 22, q).astype(np.uint32)).view(np.float32) * np.where(rng.random(q) < 0.5, -1, 1).astype(np.float32)   # denormals
    flat[idx[2 * q:3 * q]] = rng.uniform(3.0e38, 3.3e38, q).astype(np.float32)
    last = t[ntiles - 1].reshape(-1)
    last[rng.permutation(last.size)[: max(last.size // 40, 4)]] = np.nan
    return t
