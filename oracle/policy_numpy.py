"""Independent float64 restatement of the early-fixing policy network in numpy.  TEST INFRASTRUCTURE ONLY.

Written from the reference source alone (LP/mha.py and LP/common/utils.py; SEG/mha.py is the same network with 5 tokens), not from
lpbox_hip/policy.py, so that the two can pin each other: no folded position bias, no fused Q|K|V matrix, no folded BatchNorm.
  position code          utils.py:20-32   pos / 10000^(2 (j//2) / d), position 0 all zeros BEFORE sin / cos, cast to float32
  GraphAttentionEncoder  mha.py:224-249   cat([x, code]) (10 values per token) -> init_embed (Linear) -> layers -> flatten -> classify
  MultiHeadAttention     mha.py:58-122    per head h: Q = x W_query[h], K = x W_key[h], V = x W_val[h], softmax(Q K^T / sqrt(16)) V,
                                          the heads' outputs side by side times W_out viewed as (8*16, 128) = sum_h head_h W_out[h]
  layer                  mha.py:157-183   x + attention -> BatchNorm1d -> x + Linear(relu(Linear(x))) -> BatchNorm1d
  BatchNorm1d (eval)                      (h - running_mean) / sqrt(running_var + 1e-5) * weight + bias
  Net2                   mha.py:185-199   fc1 relu fc2 relu fc3 relu fc4, sigmoid

Everything is float64 with numpy's pairwise / BLAS sums: the restatement differs from exact arithmetic by float64 rounding only, which
is nine orders below the float32 error of anything it is compared with."""
import numpy as np

N_HEADS, KEY_DIM, N_LAYERS, CODE_DIM, BN_EPS = 8, 16, 2, 5, 1e-5


def position_code(n_pos, d=CODE_DIM):
    pe = np.array([[pos / np.power(10000, 2 * (j // 2) / d) for j in range(d)] if pos != 0 else np.zeros(d) for pos in range(n_pos)])
    pe[:, 0::2] = np.sin(pe[:, 0::2])
    pe[:, 1::2] = np.cos(pe[:, 1::2])
    return pe.astype(np.float32).astype(np.float64)          # the reference hands the code to the network as a FloatTensor


def _f64(state_dict, name):
    v = state_dict[name]
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64)


def _linear(state_dict, name, x):
    w = _f64(state_dict, name + ".weight")
    return (x.reshape(-1, x.shape[-1]) @ w.T).reshape(x.shape[:-1] + (w.shape[0],)) + _f64(state_dict, name + ".bias")


def _batchnorm(state_dict, name, h):
    g = lambda k: _f64(state_dict, name + ".normalizer." + k)
    return (h - g("running_mean")) / np.sqrt(g("running_var") + BN_EPS) * g("weight") + g("bias")


def _attention(state_dict, name, h):
    wq, wk, wv, wo = (_f64(state_dict, name + "." + k) for k in ("W_query", "W_key", "W_val", "W_out"))
    out = np.zeros_like(h)
    for hd in range(N_HEADS):
        q, k, v = ((h.reshape(-1, h.shape[-1]) @ w).reshape(h.shape[0], h.shape[1], -1) for w in (wq[hd], wk[hd], wv[hd]))   # (rows, T, 16) each
        c = (1.0 / np.sqrt(KEY_DIM)) * (q @ k.transpose(0, 2, 1))               # (rows, query, key)
        c = np.exp(c - c.max(axis=-1, keepdims=True))
        attn = c / c.sum(axis=-1, keepdims=True)
        out += (attn @ v) @ wo[hd]
    return out


def forward(state_dict, x, intermediates=None):
    """state_dict: GraphAttentionEncoder().state_dict() (tensors or arrays); x: (rows, T, 5).
    Returns (encoder output (rows, T*128), logits (rows,), sigmoid (rows,)), float64.  `intermediates`: an optional dict that receives
    the activations after every stage ("embed", "l0.attn", "l0.bn1", "l0.ff", "l0.bn2", ..., "fc1" .. "fc3"), for localising a difference."""
    x = np.asarray(x, dtype=np.float64)
    rows, T, c = x.shape
    assert c == CODE_DIM
    keep = intermediates if intermediates is not None else {}
    xin = np.concatenate([x, np.broadcast_to(position_code(T), (rows, T, CODE_DIM))], axis=-1)
    h = keep["embed"] = _linear(state_dict, "init_embed", xin)
    for i in range(N_LAYERS):
        p = "layers.%d." % i
        h = keep["l%d.attn" % i] = h + _attention(state_dict, p + "0.module", h)
        h = keep["l%d.bn1" % i] = _batchnorm(state_dict, p + "1", h)
        h = keep["l%d.ff" % i] = h + _linear(state_dict, p + "2.module.2", np.maximum(_linear(state_dict, p + "2.module.0", h), 0.0))
        h = keep["l%d.bn2" % i] = _batchnorm(state_dict, p + "3", h)
    enc = h.reshape(rows, -1)
    logit, sig = head(state_dict, enc, keep)
    return enc, logit, sig


def head(state_dict, enc, intermediates=None):
    """Net2 alone: encoder output (rows, T*128) -> (logits, sigmoid)."""
    keep = intermediates if intermediates is not None else {}
    z = np.asarray(enc, dtype=np.float64)
    for k in (1, 2, 3):
        z = keep["fc%d" % k] = np.maximum(_linear(state_dict, "classify.fc%d" % k, z), 0.0)
    logit = _linear(state_dict, "classify.fc4", z).reshape(z.shape[0])
    return logit, 1.0 / (1.0 + np.exp(-logit))


def tokens_from_flat(flat, row_off, tok_stride, tokens):
    """x (rows, tokens, 5) the way the kernels read the solver's iterate buffer: token t of row r = flat[row_off[r] + t*tok_stride : +5]."""
    flat = np.asarray(flat, dtype=np.float64).ravel()
    idx = np.asarray(row_off, dtype=np.int64)[:, None, None] + np.arange(tokens)[None, :, None] * int(tok_stride) + np.arange(CODE_DIM)[None, None, :]
    assert idx.min() >= 0 and idx.max() < flat.size
    return flat[idx]


def rel_err(got, want):
    """The error measure of the policy tests: |got - want| / (|want| + rms(want)), element-wise."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / (np.abs(want) + np.sqrt(np.mean(want * want)))
