"""Plain float64 statement of `srl_gae_scan` (csrc/gae.hip; the formulas in include/srl_hip.h), in numpy, together with what a
tight bound on the kernel needs.  No GPU and no project code.

`gae` is the sequential recurrence adv[t] = delta[t] + m[t] * adv[t+1] in float64, unrounded, next to the same recurrence on
absolute values, A[t] = |delta[t]| + |m[t]| * A[t+1].  Every partial quantity any association order of the scan can form -- a
chunk's folded (M, D), a suffix composite, a carry -- is a sum of products that A[t] bounds term by term, also when c > 1 makes
|m| > 1.  So a float64 evaluation in ANY order, kernel or reference, is off by at most a few 2^-53 of A per operation.

The bound on a written element (`bound`):

    |adv_gpu - g| <= 2^-24 |g| + 4 T 2^-53 A

one float32 rounding, plus the float64 rounding of kernel and reference together over at most 2 T operations each.  Nothing in it
is measured.

`scan_in_tiles` is the kernels' evaluation order in numpy float64 (time tiles from the end, chunks folded into affine maps, the
carry-in of a chunk from the maps behind it, the replay, the carry across tiles).  It runs on the host only: it shows that
re-association alone stays inside the float64 term, and it is where the deliberate faults of the scan are injected.  `FAULTS` are
deliberate errors, of the inputs (`gae(..., fault=)`) or of the scan (`scan_in_tiles(..., fault=)`), used only to show that the
bound can fail (tests/test_gae_reference.py)."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53

INPUT_FAULTS = ("no_done_mask", "done_rotated_in_quad", "truncated_ignored", "on_reset_same_row", "rho_c_swapped",
                "tensors_from_tile_row0", "flag_col_not_divided")
SCAN_FAULTS = ("carry_zeroed_at_tile_seam", "carry_from_wrong_chunk")
FAULTS = INPUT_FAULTS + SCAN_FAULTS


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _flag_rows(flag, Nc, fault):
    """A [T+1, B, 1] flag as the columns (env, channel) see it: [T+1, B, 1], or with `flag_col_not_divided` [T+1, B, Nc] read at
    the flat index t * B + col, col = env * Nc + channel, the way a kernel that forgot `col / Nc` would (clipped to the leaf)."""
    flag = np.asarray(flag)
    if fault != "flag_col_not_divided":
        return flag
    Tp1, B = flag.shape[:2]
    idx = np.arange(Tp1)[:, None] * B + np.arange(B * Nc)[None, :]
    return flag.reshape(-1)[np.minimum(idx, flag.size - 1)].reshape(Tp1, B, Nc)


def gae(reward, value, done, truncated, on_reset, gamma, lmbda, ratio=None, rho=1.0, c=1.0, fault=None, TT=None):
    """reward [>= T, B, Nc] float32 (rows 0..T-1 read); value [T+1, B, Nc] float32, raw: the masking float32(value) * (1 - done)
    happens here, in float32 (mappo.py:124); done / truncated / on_reset [T+1, B, 1]; gamma / lmbda python floats or [T, B, 1]
    float32 arrays (widened to float64, gae.py:51-60); ratio [T, B, 1] float32 or None (V-trace with clamps rho, c).
    Returns a dict of float64 arrays [T, B, Nc] -- g (the unrounded advantage), A (the recurrence on absolute values), delta, m --
    and v, the float32 masked value [T+1, B, Nc].  `fault`: one of INPUT_FAULTS (`tensors_from_tile_row0` needs the time tile TT)."""
    assert fault is None or fault in INPUT_FAULTS, fault
    value = np.asarray(value, np.float32)
    Tp1, B, Nc = value.shape
    T = Tp1 - 1
    dn = _flag_rows(done, Nc, fault)
    if fault == "done_rotated_in_quad":   # every column masks by the done byte of its neighbour in the quad
        dn = np.roll(np.asarray(done).reshape(Tp1, B // 4, 4), 1, axis=2).reshape(Tp1, B, 1)
    if fault == "no_done_mask":
        dn = np.zeros_like(dn)
    v = (value * (1 - dn.astype(np.float32))).astype(np.float32)
    orr = _f64(_flag_rows(on_reset, Nc, fault))
    nr = 1.0 - (orr[:-1] if fault == "on_reset_same_row" else orr[1:])
    nt = 1.0 - _f64(_flag_rows(truncated, Nc, fault))[1:]
    if fault == "truncated_ignored":
        nt = np.ones_like(nt)

    def per_step(x):
        if isinstance(x, float):
            return x
        x = _f64(x)
        assert x.shape == (T, B, 1), x.shape
        if fault == "tensors_from_tile_row0":   # staged from the leaf's row 0 in every tile, not from the tile's first row t0
            rows = np.arange(T)
            for t1 in range(T, 0, -TT):
                t0 = max(t1 - TT, 0)
                rows[t0:t1] -= t0
            x = x[rows]
        return x

    gam, lam = per_step(gamma), per_step(lmbda)
    delta = _f64(reward)[:T] + gam * _f64(v[1:]) * nr - _f64(v[:-1])   # gae.py:63
    m = gam * lam * nr * nt                                             # gae.py:87
    if ratio is not None:
        q = _f64(ratio)
        if fault == "rho_c_swapped":
            rho, c = c, rho
        delta = delta * np.minimum(q, rho)                              # gae.py:65
        m = m * np.minimum(q, c)                                        # gae.py:89
    m = np.broadcast_to(m, delta.shape)
    g, A = np.zeros_like(delta), np.zeros_like(delta)
    run, run_abs = np.zeros(delta.shape[1:]), np.zeros(delta.shape[1:])
    for t in range(T - 1, -1, -1):                                      # gae.py:91-95
        run = delta[t] + m[t] * run
        run_abs = np.abs(delta[t]) + np.abs(m[t]) * run_abs
        g[t], A[t] = run, run_abs
    return dict(g=g, A=A, delta=delta, m=np.array(m), v=v)


def bound(g, A, T):
    """The admissible |adv_gpu - g| per element: one float32 rounding of g, and the float64 rounding of both evaluations."""
    return U32 * np.abs(g) + f64_term(A, T)


def f64_term(A, T):
    return 4.0 * T * U64 * A


def scan_in_tiles(delta, m, SEG, L, TT=None, log_step=True, fault=None):
    """g [T, ...] of the recurrence in the kernels' order, float64.  Time tiles of TT rows (default SEG * L) taken from the end;
    in a tile every one of SEG chunks of L consecutive rows is folded into an affine map g_a = D + M g_b (rows past a partial
    tile: the identity); the carry-in of chunk s is the composite of the chunks behind it applied to the tile's carry; the chunk is
    replayed from it; the whole tile applied to the carry is the next tile's carry.

    The register kernel: L is 1, 2 or 4, TT = SEG * L, the composites come from a log-step inclusive suffix scan over the chunk
    maps (`log_step`).  The LDS kernel: L=None, a chunk of a tile of len rows has ceil(len / SEG) rows, the carry-in is folded
    sequentially from the last chunk down (`log_step=False`).  `fault`: one of SCAN_FAULTS."""
    assert fault is None or fault in SCAN_FAULTS, fault
    delta, m = _f64(delta), _f64(m)
    T, cols = delta.shape[0], delta.shape[1:]
    TT = SEG * L if TT is None else TT
    g = np.zeros_like(delta)
    carry = np.zeros(cols)
    for t1 in range(T, 0, -TT):
        t0 = max(t1 - TT, 0)
        n = t1 - t0
        Lc = L if L is not None else -(-n // SEG)
        d_t = np.zeros((SEG * Lc,) + cols)
        m_t = np.ones((SEG * Lc,) + cols)
        d_t[:n], m_t[:n] = delta[t0:t1], m[t0:t1]
        d_t, m_t = d_t.reshape((SEG, Lc) + cols), m_t.reshape((SEG, Lc) + cols)
        # pass 1: fold every chunk
        M, D = np.ones((SEG,) + cols), np.zeros((SEG,) + cols)
        for i in range(Lc - 1, -1, -1):
            D = d_t[:, i] + m_t[:, i] * D
            M = m_t[:, i] * M
        # pass 2: carry-in of every chunk
        cin = np.empty((SEG,) + cols)
        if log_step:
            off = 1
            while off < SEG:   # inclusive suffix scan, in place, all chunks at once
                M2, D2 = np.ones_like(M), np.zeros_like(D)
                M2[:SEG - off], D2[:SEG - off] = M[off:], D[off:]
                D, M = D + M * D2, M * M2
                off <<= 1
            Mn, Dn = np.ones_like(M), np.zeros_like(D)   # composite of the chunks strictly behind s
            k = 2 if fault == "carry_from_wrong_chunk" else 1
            Mn[:max(SEG - k, 0)], Dn[:max(SEG - k, 0)] = M[k:], D[k:]
            cin = Dn + Mn * carry
            out = D[0] + M[0] * carry
        else:
            run = carry
            skip = 1 if fault == "carry_from_wrong_chunk" else 0   # chunk s starts from the carry-in of chunk s + 1
            runs = [None] * (SEG + 1)
            for s in range(SEG - 1, -1, -1):
                runs[s + 1] = run          # the value entering chunk s from behind
                run = D[s] + M[s] * run
            for s in range(SEG):
                cin[s] = runs[min(s + 1 + skip, SEG)]
            out = run
        # pass 3: replay
        run = cin
        g_t = np.empty_like(d_t)
        for i in range(Lc - 1, -1, -1):
            run = d_t[:, i] + m_t[:, i] * run
            g_t[:, i] = run
        g[t0:t1] = g_t.reshape((SEG * Lc,) + cols)[:n]
        carry = np.zeros(cols) if fault == "carry_zeroed_at_tile_seam" else out
    return g


def stats(adv_f32, on_reset):
    """{n, s, q, sabs}: sum mask, sum x, sum x^2 and sum |x| with x = adv * mask in float64, mask[t] = 1 - on_reset[t+1].  The mask is
    [T, B, 1]: n counts every (step, env) once, the other sums run over all value channels (utils.py:41-55)."""
    adv = _f64(adv_f32)
    T = adv.shape[0]
    mask = 1.0 - _f64(on_reset)[1:T + 1]
    x = adv * mask
    return dict(n=float(mask.sum()), s=float(x.sum()), q=float((x * x).sum()), sabs=float(np.abs(x).sum()))
