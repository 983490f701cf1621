"""A plain restatement of one chunk of the auto-reset recurrent layer (LSTM / GRU), buffer by buffer as the HIP kernels see it
(csrc/rnn_seq.hip, csrc/gru.hip, `srl_amd/algorithm/rnnpath.py`), in torch on the CPU with autograd for the backward.

Run in float64 it is the reference the kernels are held to (tests/test_gpu_rnn.py); run in float32 it measures how far an honest
float32 evaluation of the same arithmetic lands from float64, which sets the tolerance.  tests/test_rnn_reference.py holds it
against torch.nn.LSTM / torch.nn.GRU.

One chunk of C steps over N independent rows (environment columns):
  the state entering step c is h * (1 - reset[c]) (autoreset_rnn.py:59), hin[0] from the stored state h0 / c0;
  LSTM  pre = W_ih x + b_ih + W_hh h + b_hh, gates i | f | g | o: c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c');
  GRU   gi = W_ih x + b_ih, gh = W_hh h + b_hh, gates r | z | n: n = tanh(gi_n + r * gh_n), h' = (1 - z) n + z h.
`FAULTS` are deliberate errors of this restatement, used only to show that the tolerances can fail.  `check_vs_float64` holds a
whole recurrent net's device step to the float64 oracle (oracle/net.py)."""
import torch

FAULTS = ("reset_late", "carry_not_cut", "bhn_outside", "if_swap", "row_dropped")


def chunk(kind, pre_x, w_hh, b_hh, h0, c0, reset, dy, fault=None):
    """kind "lstm" / "gru"; pre_x [C, N, G H] = W_ih x + b_ih of every step; w_hh [G H, H]; b_hh [G H] or None; h0, c0 [N, H]
    stored states (c0 unused by a GRU); reset [C, N] (0 / 1) or None; dy [C, N, H] = d loss / d y.  Computes in the dtype of
    pre_x and returns what the kernels write, each [C, N, ...]:
      gates (activated gates), gh (GRU: W_hh h + b_hh), hin / cin (the masked states entering each step), y, cnew (LSTM: c');
      d_pre (LSTM d pre / GRU d gi), d_gh (GRU), d_hin / d_cin (d loss / d state entering each step: the per-step carries)."""
    dt = pre_x.dtype
    C, N, _ = pre_x.shape
    H = w_hh.shape[1]
    pre_x = pre_x.detach().clone().requires_grad_(True)
    w_hh = w_hh.to(dt)
    b_hh = torch.zeros(w_hh.shape[0], dtype=dt) if b_hh is None else b_hh.to(dt)
    keep = torch.ones(C, N, 1, dtype=dt) if reset is None else 1 - reset.to(dt).reshape(C, N, 1)
    if fault == "reset_late":   # the mask of step c applied at step c + 1
        keep = torch.cat([torch.ones(1, N, 1, dtype=dt), keep[:-1]], 0)

    def mask(v, c):
        if fault == "carry_not_cut":   # the forward value is cut, the gradient is not
            return torch.where(keep[c] > 0, v, v - v.detach())
        return v * keep[c]

    h, cs = h0.to(dt).detach().requires_grad_(True), c0.to(dt).detach().requires_grad_(True)
    out = {k: [] for k in ("gates", "gh", "hin", "cin", "y", "cnew")}
    for c in range(C):
        h = mask(h, c)
        h.retain_grad()
        out["hin"].append(h)
        if kind == "lstm":
            cs = mask(cs, c)
            cs.retain_grad()
            out["cin"].append(cs)
            i, f, g, o = (pre_x[c] + h @ w_hh.T + b_hh).chunk(4, -1)
            if fault == "if_swap":
                i, f = f, i
            gi_, gf, gg, go = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            cs = gf * cs + gi_ * gg
            h = go * torch.tanh(cs)
            out["gates"].append(torch.cat([gi_, gf, gg, go], -1))
            out["cnew"].append(cs)
        else:
            if fault == "bhn_outside":
                gh = h @ w_hh.T + torch.cat([b_hh[:2 * H], torch.zeros(H, dtype=dt)])
            else:
                gh = h @ w_hh.T + b_hh
            gh.retain_grad()
            ir, iz, inn = pre_x[c].chunk(3, -1)
            hr, hz, hn = gh.chunk(3, -1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            n = torch.tanh(inn + r * hn + (b_hh[2 * H:] if fault == "bhn_outside" else 0))
            h = (1 - z) * n + z * h
            out["gates"].append(torch.cat([r, z, n], -1))
            out["gh"].append(gh)
        out["y"].append(h)
    y = torch.stack(out["y"])
    (y * dy.to(dt)).sum().backward()
    res = {k: torch.stack(v).detach() for k, v in out.items() if v}
    res["d_pre"] = pre_x.grad.detach()
    res["d_hin"] = torch.stack([t.grad if t.grad is not None else torch.zeros_like(t) for t in out["hin"]])
    if kind == "lstm":
        res["d_cin"] = torch.stack([t.grad if t.grad is not None else torch.zeros_like(t) for t in out["cin"]])
    else:
        res["d_gh"] = torch.stack([t.grad for t in out["gh"]])
    if fault == "row_dropped":   # a kernel that skips the last row of the last (ragged) tile leaves it as it was: zero here
        for v in res.values():
            v[:, N - 1] = 0
    return res


def check_vs_float64(stats, grads, oracles, stat_keys, bias_floor=2e-6):
    """The device step's loss terms and gradients against the float64 oracle: error <= 3 x the float32 oracle's + 2e-6 x the
    tensor's largest element (`bias_floor` x for biases: a bias's gradient is a column sum over all rows, see the SMAC test).
    Returns the largest ratio of error to bound."""
    (o32, s32), (o64, s64) = oracles[torch.float32], oracles[torch.float64]
    rows = [(k, abs(stats[k] - s64[k]), abs(s32[k] - s64[k]), 2e-6 * abs(s64[k])) for k in stat_keys]
    for k, p in o64.params.items():
        if p.grad is not None:
            g64 = p.grad.double()
            floor = bias_floor if "bias" in k.rpartition(".")[2] else 2e-6
            rows.append((k, float((grads[k].double() - g64).abs().max()), float((o32.params[k].grad.double() - g64).abs().max()),
                         floor * float(g64.abs().max())))
    ratios = sorted((e / max(3 * e32 + fl, 1e-300), k, e, e32, fl) for k, e, e32, fl in rows)
    print("\nworst error / bound against float64:", ratios[-3:])
    assert ratios[-1][0] <= 1.0, [r for r in ratios if r[0] > 1.0]
    return ratios[-1][0]
