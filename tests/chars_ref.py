"""numpy restatement of the character-box rule (DESIGN.md "Character boxes"; geometry.cpp: chars_coef, chars_profile,
chars_cuts_from_profile, chars_quads_from_cuts; chars.hip: char_cut_kernel).  The integer outputs (cuts, mode, profile) are exact, so the
tests compare them with np.array_equal.  Also the generators of the CPU and GPU suites: random maps and quads, and the hand-made words of
Gaussian blobs whose character centres are known."""
import numpy as np

U, V, LAM, MAXK = 128, 16, 64, 26
INF = 0x3FFFFFFF


def scale(ratio):
    """k = 1 / (double)(ratio_w * 2.f), ratio_w = 1.f / ratio: image pixels -> heat pixels"""
    ratio_w = np.float32(1.0) / np.float32(ratio)
    return 1.0 / float(np.float32(ratio_w * np.float32(2.0)))


def coef(quad, turn, k):
    """one quad f32 [8] (tl, tr, br, bl) at turn t -> int64 {X0, Ax, Bx, Y0, Ay, By} in 2^-16 heat pixels, or None when refused"""
    q = np.asarray(quad, np.float32).reshape(4, 2)
    if not (k > 0.0 and k <= 1024.0) or not np.isfinite(q).all() or (np.abs(q) >= np.float32(32768.0)).any():
        return None
    p = q[(np.arange(4) + turn) % 4].astype(np.float64)
    tl, tr, bl = p[0], p[1], p[3]
    out = []
    for a in range(2):
        A, B = tr[a] - tl[a], bl[a] - tl[a]
        Au, Bv = (A * k) / U, (B * k) / V
        x0 = (tl[a] * k + 0.5 * Au) + 0.5 * Bv
        out += [int(np.rint(65536.0 * x0)), int(np.rint(65536.0 * Au)), int(np.rint(65536.0 * Bv))]
    return np.array(out, np.int64)


def profile(T, fx):
    """q u8 [128]: per column the maximum of 16 samples of T (clamped to the map; a NaN loses), times 255 in f32, truncated"""
    T = np.asarray(T, np.float32)
    H2, W2 = T.shape
    u = np.arange(U, dtype=np.int64)[:, None]
    v = np.arange(V, dtype=np.int64)[None, :]
    ix = np.clip((fx[0] + u * fx[1] + v * fx[2] + 32768) >> 16, 0, W2 - 1)
    iy = np.clip((fx[3] + u * fx[4] + v * fx[5] + 32768) >> 16, 0, H2 - 1)
    s = T[iy, ix]
    P = s[:, 0]
    for j in range(1, V):
        P = np.fmax(P, s[:, j])
    with np.errstate(invalid="ignore", over="ignore"):
        val = np.fmin(np.fmax(P, np.float32(0.0)) * np.float32(255.0), np.float32(255.0))
    return val.astype(np.int32).astype(np.uint8)


def cuts_from_profile(q, K, qlow):
    """q u8 [128], K, qlow -> (cuts i32 [27], mode)"""
    q = np.asarray(q).astype(np.int64).reshape(U)
    cuts = np.full(MAXK + 1, -1, np.int32)
    if K <= 0:
        return cuts, 0
    ink = np.nonzero(q > qlow)[0]
    u0, u1 = (int(ink[0]), int(ink[-1]) + 1) if len(ink) else (0, U)
    L = u1 - u0
    if not len(ink) or L < 2 * K:
        for j in range(K + 1):
            cuts[j] = 256 * u0 + (256 * L * j) // K
        return cuts, 0
    wlo, whi = max(1, L // (2 * K)), min(L, (2 * L + K - 1) // K)
    prev = np.full(U + 1, INF, np.int64)
    prev[u0] = 0
    arg = np.zeros((MAXK + 1, U + 1), np.int64)
    g = np.zeros(U + 1, np.int64)
    g[1:U] = q[:-1] + q[1:]
    for j in range(1, K + 1):
        cur = np.full(U + 1, INF, np.int64)
        for c in ([u1] if j == K else range(u0 + 1, u1 + 1)):
            lo, hi = max(u0, c - whi), c - wlo
            if hi < lo:
                continue
            cp = np.arange(lo, hi + 1)
            dev = np.abs((c - cp) * K - L)
            cost = prev[cp] + (g[cp] if j > 1 else 0) + (LAM * dev) // L
            cost = np.where(prev[cp] >= INF, INF, cost)
            i = int(np.argmin(cost))                       # the first minimum: ties go to the smallest c'
            if cost[i] < INF:
                cur[c], arg[j][c] = cost[i], cp[i]
        prev = cur
    c = u1
    for j in range(K, 0, -1):
        cuts[j] = 256 * c
        c = int(arg[j][c])
    cuts[0] = 256 * c
    return cuts, 1


def chars_from_map(T, ratio, low_text, quads, turns, nchars):
    """the whole rule on n words of one plane -> (cuts [n, 27], mode [n], profile [n, 128]); None when a quad is refused"""
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    n = len(quads)
    k = scale(ratio)
    qlow = int(np.float32(low_text) * np.float32(255.0))
    cuts, modes, prof = np.zeros((n, MAXK + 1), np.int32), np.zeros(n, np.int32), np.zeros((n, U), np.uint8)
    for i in range(n):
        fx = coef(quads[i], int(turns[i]), k)
        if fx is None:
            return None
        prof[i] = profile(T, fx)
        cuts[i], modes[i] = cuts_from_profile(prof[i], int(nchars[i]), qlow)
    return cuts, modes, prof


def quads_from_cuts(quad, turn, cuts, K):
    """the K cells in float64: (quads [K, 8], bboxes [K, 4])"""
    p = np.asarray(quad, np.float32).reshape(4, 2)[(np.arange(4) + turn) % 4].astype(np.float64)
    tl, tr, br, bl = p
    out = np.zeros((K, 8)); bb = np.zeros((K, 4))
    for j in range(K):
        t0, t1 = cuts[j] / 32768.0, cuts[j + 1] / 32768.0
        c = np.stack([tl + t0 * (tr - tl), tl + t1 * (tr - tl), bl + t1 * (br - bl), bl + t0 * (br - bl)])
        out[j] = c.reshape(8)
        bb[j] = [c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()]
    return out, bb


# ---------------------------------------------------------------- generators
def rect_quad(cx, cy, w, h, deg):
    """tl, tr, br, bl of a w x h rectangle about (cx, cy), its baseline tilted by deg (y down)"""
    a = np.deg2rad(deg)
    ux, uy = np.cos(a), np.sin(a)
    vx, vy = -uy, ux
    c = np.array([cx, cy])
    u, v = np.array([ux, uy]) * w / 2, np.array([vx, vy]) * h / 2
    return np.stack([c - u - v, c + u - v, c + u + v, c - u + v]).astype(np.float32).reshape(8)


def random_map(seed, H2, W2):
    rng = np.random.default_rng(seed)
    t = rng.random((H2, W2), dtype=np.float32)
    yy, xx = np.mgrid[0:H2, 0:W2]
    t *= (0.5 + 0.5 * np.sin(xx / 3.0) * np.cos(yy / 5.0)).astype(np.float32)      # blobs and valleys rather than white noise alone
    t[rng.integers(0, H2), rng.integers(0, W2)] = np.nan
    t[rng.integers(0, H2), rng.integers(0, W2)] = np.inf
    t[rng.integers(0, H2), rng.integers(0, W2)] = -1.0
    return t


def random_words(seed, n, H2, W2, ratio, outside=False):
    """n quads in image pixels over a map of H2 x W2 heat pixels: tilted to 44 degrees, every turn; outside=True lets them leave the map"""
    rng = np.random.default_rng(seed)
    k = scale(ratio)
    quads = np.zeros((n, 8), np.float32)
    for i in range(n):
        w, h = rng.uniform(20, 300), rng.uniform(8, 60)
        m = -0.3 if outside else 0.1
        cx, cy = rng.uniform(m * W2, (1 - m) * W2) / k, rng.uniform(m * H2, (1 - m) * H2) / k
        q = rect_quad(cx, cy, w, h, rng.uniform(-44, 44)).reshape(4, 2)
        quads[i] = np.roll(q, -int(rng.integers(0, 4)), axis=0).reshape(8)          # the word lies on the page at any quarter turn
    turns = rng.integers(0, 4, n).astype(np.int32)
    nchars = rng.choice(np.array([0, 1, 2, 3, 5, 7, 13, 26]), n).astype(np.int32)
    return quads, turns, nchars


def blob_words(seed, k, count):
    """Hand-made words for the functional test: each word is K Gaussian blobs on its own half-resolution map, all sizes in map pixels
    (height 20..48, character widths 0.3..0.9 of it, a word longer than 400 is dropped); the quad is the word's box in image pixels (map / k).
    Yields (T f32 [H2, W2], ratio, quad f32 [8] in image pixels, K, centres [K] as fractions of the baseline)."""
    rng = np.random.default_rng(seed)
    ratio = 2.0 * k
    assert abs(scale(ratio) - k) < 1e-12
    for _ in range(count):
        K = int(rng.integers(2, 13))
        h = rng.uniform(20, 48)
        widths = rng.uniform(0.3, 0.9, K) * h
        deg = rng.uniform(-40, 40)
        amps = rng.uniform(0.75, 0.95, K)
        Lw = widths.sum()
        if Lw > 400:
            continue
        a = np.deg2rad(deg)
        ext_x = (abs(np.cos(a)) * Lw + abs(np.sin(a)) * h) / 2 + 4
        ext_y = (abs(np.sin(a)) * Lw + abs(np.cos(a)) * h) / 2 + 4
        W2, H2 = int(np.ceil(2 * ext_x)) + 2, int(np.ceil(2 * ext_y)) + 2
        cx, cy = W2 / 2.0, H2 / 2.0
        u = np.array([np.cos(a), np.sin(a)]); v = np.array([-u[1], u[0]])
        edges = np.concatenate([[0.0], np.cumsum(widths)])
        mids = (edges[:-1] + edges[1:]) / 2                     # along the baseline, from the word's left end
        yy, xx = np.mgrid[0:H2, 0:W2].astype(np.float64)
        du = (xx - cx) * u[0] + (yy - cy) * u[1]                # along / across the baseline, from the word's centre
        dv = (xx - cx) * v[0] + (yy - cy) * v[1]
        T = np.zeros((H2, W2))
        for j in range(K):
            su, sv = 0.32 * widths[j], 0.32 * h
            T = np.maximum(T, amps[j] * np.exp(-0.5 * (((du - (mids[j] - Lw / 2)) / su) ** 2 + (dv / sv) ** 2)))
        T = T + rng.normal(0.0, 0.03, T.shape)
        quad = rect_quad(cx / k, cy / k, Lw / k, h / k, deg)    # pixel centres at integers: map = image * k
        yield T.astype(np.float32), ratio, quad, K, mids / Lw
