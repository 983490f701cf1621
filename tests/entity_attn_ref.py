"""A plain restatement of the agent-specific attention encoder as the HIP kernel sees it (csrc/entity_attn.hip, include/srl_hip.h:
srl_entity_attn_*), in torch on the CPU with autograd for the backward, and the seeded cases the kernel is held to beyond a
workgroup's first tile (tests/test_gpu_entity_attn.py).

Run in float64 it is the reference; run in float32 it measures how far an honest float32 evaluation of the same arithmetic lands
from float64, which sets the tolerance (tests/rnn_ref.py).  tests/test_entity_attn_reference.py holds it against the golden blocks
of the real reference (tests/golden/steps_smac_attn.npz).

Per row: a_s = LayerNorm(x_self), a_e = LayerNorm(x_e) (eps 1e-5, affine, one pair of affines per leaf);
  self_emb = relu(W_s a_s + b_s);  emb_e = relu(W_k cat(a_s, a_e) + b_k) in leaf order;  xn = pre_norm(emb);
  q, k, v = Linear(xn); 4 heads of D / 4; s = q k^T / sqrt(D / 4) - 1e10 (1 - mask_key); s -= max_key s; p = softmax(s) * mask_key;
  o = p v;  pooled = sum_e mask_e o_e / (sum_e mask_e + 1e-5);  out = cat(self_emb, pooled).
Parameters go by the reference's names (test_gpu_smac_attn.py::SLOTS): ``obs_self_norm``, ``<leaf>_norm``,
``encoder.embedding.self_embedding.0``, ``encoder.embedding.<leaf>_fc.0``, ``encoder.attn.pre_norm`` / ``q_linear`` / ``k_linear`` /
``v_linear``, each ``.weight`` and ``.bias``.
`FAULTS` are deliberate errors of this restatement, used only to show that the tolerances can fail."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

FAULTS = ("later_tiles_dropped", "last_row_dropped", "masked_query_pooled", "pool_eps_missing")
HEADS = 4
ATTN = "encoder.attn."


def leaf_names(n):
    return [f"obs_leaf{i}" for i in range(n)]


def preactivations(p, x_self, x_keys, keys):
    """(a_s, z_self [n, D], z_ent [n, E, D]): the embeddings before their ReLU, in the dtype of ``p``."""
    a_s = F.layer_norm(x_self, x_self.shape[-1:], p["obs_self_norm.weight"], p["obs_self_norm.bias"], 1e-5)
    z_self = F.linear(a_s, p["encoder.embedding.self_embedding.0.weight"], p["encoder.embedding.self_embedding.0.bias"])
    z = []
    for k, x in zip(keys, x_keys):
        a = F.layer_norm(x, x.shape[-1:], p[f"{k}_norm.weight"], p[f"{k}_norm.bias"], 1e-5)
        cat = torch.cat([a_s.unsqueeze(1).expand(-1, x.shape[1], -1), a], -1)
        z.append(F.linear(cat, p[f"encoder.embedding.{k}_fc.0.weight"], p[f"encoder.embedding.{k}_fc.0.bias"]))
    return a_s, z_self, torch.cat(z, 1)


def encoder(params, x_self, x_keys, mask, cot, keys, dtype, fault=None, fault_row=None):
    """params: name -> array; x_self [n, S]; x_keys: one [n, entities, features] per leaf of ``keys``; mask [n, E] (0 / non-zero);
    cot [n, 2 D] = d loss / d out.  Computes in ``dtype`` and returns numpy arrays:
    out [n, 2 D], {name: gradient}, z_self [n, D], z_ent [n, E, D] (the embeddings' pre-activations)."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    p = OrderedDict((k, t(v).clone().requires_grad_(True)) for k, v in params.items())
    x_self, x_keys, cot = t(x_self), [t(x) for x in x_keys], t(cot)
    m = (torch.as_tensor(np.asarray(mask)) != 0).to(dtype)
    n, D = x_self.shape[0], p[ATTN + "pre_norm.weight"].shape[0]
    dh = D // HEADS
    _, z_self, z_ent = preactivations(p, x_self, x_keys, keys)
    E = z_ent.shape[1]
    xn = F.layer_norm(torch.relu(z_ent), (D,), p[ATTN + "pre_norm.weight"], p[ATTN + "pre_norm.bias"], 1e-5)
    heads = lambda name: F.linear(xn, p[ATTN + name + ".weight"], p[ATTN + name + ".bias"]).view(n, E, HEADS, dh).transpose(1, 2)
    q, k, v = heads("q_linear"), heads("k_linear"), heads("v_linear")
    mk = m.view(n, 1, 1, E)
    s = q @ k.transpose(-1, -2) / math.sqrt(dh) - (1 - mk) * 1e10
    s = s - s.max(-1, keepdim=True)[0]
    o = ((torch.softmax(s, -1) * mk) @ v).transpose(1, 2).reshape(n, E, D)
    mq = torch.ones_like(m) if fault == "masked_query_pooled" else m          # pooling ignores the query's mask
    den = m.sum(-1, keepdim=True)
    den = den.clamp(min=1.0) if fault == "pool_eps_missing" else den + 1e-5   # (an empty row still pools to 0)
    out = torch.cat([torch.relu(z_self), (o * mq.unsqueeze(-1)).sum(1) / den], -1)
    seen = torch.ones(n, 1, dtype=dtype)
    if fault == "later_tiles_dropped":   # rows from `fault_row` on add nothing to the gradients
        seen[fault_row:] = 0
    if fault == "last_row_dropped":      # a kernel that skips the last row of the ragged tile: no output, no gradient
        seen[n - 1] = 0
    (out * cot * seen).sum().backward()
    out = out.detach().clone()
    if fault == "last_row_dropped":
        out[n - 1] = 0
    grads = OrderedDict((k, (torch.zeros_like(v) if v.grad is None else v.grad).numpy()) for k, v in p.items())
    return out.numpy(), grads, z_self.detach().numpy(), z_ent.detach().numpy()


def keep_rows(z_self, z_ent, rel=1e-5):
    """Rows in which no embedding pre-activation of the float64 statement lies within ``rel`` x the row's max|z| of zero: a float32
    pass may take such a ReLU gate the other way, and one flipped gate moves a gradient by a whole row's share."""
    top = np.maximum(np.abs(z_self).max(-1), np.abs(z_ent).max((-1, -2)))
    low = np.minimum(np.abs(z_self).min(-1), np.abs(z_ent).min((-1, -2)))
    return low >= rel * top


# name: (D, S, [(entities, features), ...], (stage_p, stage_g) of the backward plan)
CASES = OrderedDict([
    ("staged_many_tiles", (16, 7, [(2, 5), (3, 6), (1, 4)], (1, 1))),      # R = 16, two workgroups per CU, LDS sums over 2-3 tiles
    ("staged_r1", (32, 20, [(31, 4), (32, 4), (1, 4)], (1, 1))),           # E = 64, one row per backward tile
    ("params_only", (64, 40, [(7, 4), (8, 4), (1, 4)], (1, 0))),           # gradients by global atomics on every tile, R = 2
    ("params_only_r1", (64, 40, [(15, 4), (16, 4), (1, 4)], (1, 0))),
    ("unstaged_d64", (64, 40, [(31, 4), (32, 4), (1, 4)], (0, 0))),
    ("unstaged_d32", (32, 128, [(31, 64), (32, 64), (1, 64)], (0, 0))),    # S, f, E at their limits
    ("widest", (64, 128, [(63, 64), (1, 64)], (0, 0))),                    # D = 64 at every limit
    ("one_wide_leaf", (32, 128, [(2, 64)], (1, 1))),                       # nkeys = 1; forward and backward tiles of different R
    ("smallest", (16, 1, [(1, 1)], (1, 1))),                               # S = f = E = 1
])


def draw_params(D, S, shapes, rng):
    """Weights N(0, 1 / in); LayerNorm weights 1 + 0.1 N; every bias 0.1 N.  float32."""
    keys = leaf_names(len(shapes))
    p = OrderedDict()

    def norm(name, n):
        p[name + ".weight"] = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
        p[name + ".bias"] = (0.1 * rng.standard_normal(n)).astype(np.float32)

    def linear(name, out, in_):
        p[name + ".weight"] = (rng.standard_normal((out, in_)) / np.sqrt(in_)).astype(np.float32)
        p[name + ".bias"] = (0.1 * rng.standard_normal(out)).astype(np.float32)

    norm("obs_self_norm", S)
    for k, (_, f) in zip(keys, shapes):
        norm(f"{k}_norm", f)
    linear("encoder.embedding.self_embedding.0", D, S)
    for k, (_, f) in zip(keys, shapes):
        linear(f"encoder.embedding.{k}_fc.0", D, S + f)
    norm(ATTN + "pre_norm", D)
    for name in ("q_linear", "k_linear", "v_linear"):
        linear(ATTN + name, D, D)
    return p


def draw_case(name, rows, seed, forced=()):
    """Seeded data of case ``name``, exactly ``rows`` rows: standard normal inputs and cotangent, mask bytes 1 with probability 0.7.
    1.3 x ``rows`` rows are drawn, the rows `keep_rows` refuses are dropped (by the float64 pre-activations alone: nothing of the
    code under test decides) and the first ``rows`` of the rest kept; at most 20 % may be dropped.  Then the masks of row 0, of the
    last row and of the rows ``forced`` are cleared, and row 1 keeps a single live entity.
    Returns dict(D, S, shapes, keys, params, x_self, x_keys, mask, cot, dropped)."""
    D, S, shapes, _ = CASES[name]
    rng = np.random.default_rng(seed)
    keys, E = leaf_names(len(shapes)), sum(c for c, _ in shapes)
    params = draw_params(D, S, shapes, rng)
    n = int(math.ceil(1.3 * rows))
    x_self = rng.standard_normal((n, S)).astype(np.float32)
    x_keys = [rng.standard_normal((n, c, f)).astype(np.float32) for c, f in shapes]
    mask = (rng.random((n, E)) < 0.7).astype(np.uint8)
    cot = rng.standard_normal((n, 2 * D)).astype(np.float32)
    with torch.no_grad():
        p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
        _, zs, ze = preactivations(p64, torch.from_numpy(x_self).double(), [torch.from_numpy(x).double() for x in x_keys], keys)
    keep = keep_rows(zs.numpy(), ze.numpy())
    dropped = 1.0 - keep.mean()
    assert dropped <= 0.2, (name, dropped)
    idx = np.flatnonzero(keep)[:rows]
    assert len(idx) == rows, (name, len(idx), rows)
    x_self, x_keys, mask, cot = x_self[idx], [x[idx] for x in x_keys], mask[idx].copy(), cot[idx]
    for r in (0, rows - 1, *forced):
        mask[r] = 0
    mask[1] = 0
    mask[1, E - 1] = 1
    return dict(D=D, S=S, shapes=shapes, keys=keys, params=params, x_self=x_self, x_keys=x_keys, mask=mask, cot=cot, dropped=dropped)


def zero_gradient_floors(S, shapes):
    """Tensors whose true gradient is identically zero take their floor from a named sibling: ``k_linear.bias`` (a constant added to
    every key cancels in the softmax) from ``q_linear.bias``; a LayerNorm weight over a length-1 vector (the normalised input is 0)
    from that LayerNorm's bias; with one entity (the softmax is 1 whatever q and k are) ``q_linear.*`` / ``k_linear.*`` from the
    matching ``v_linear.*``."""
    floors = {ATTN + "k_linear.bias": ATTN + "q_linear.bias"}
    if S == 1:
        floors["obs_self_norm.weight"] = "obs_self_norm.bias"
    for k, (_, f) in zip(leaf_names(len(shapes)), shapes):
        if f == 1:
            floors[f"{k}_norm.weight"] = f"{k}_norm.bias"
    if sum(c for c, _ in shapes) == 1:
        for lin in ("q_linear", "k_linear"):
            for what in ("weight", "bias"):
                floors[f"{ATTN}{lin}.{what}"] = f"{ATTN}v_linear.{what}"
    return floors

