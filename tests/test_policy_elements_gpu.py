"""GPU tests of the policy kernels at the level they compute at: every element of the encoder output against the float64 restatement
(oracle/policy_numpy.py, pinned to the reference module by tests/test_policy_restatement.py), bitwise isolation between the variables
that share a workgroup, the ragged last workgroup, the end of the output buffer, the re-score selection of policy_f32_kernel row by
row, and fix decisions on a state that HAS decisions (tests/test_policy.py's states put every score between the thresholds).

Shapes: the smallest that reach every path.  V = variables per workgroup: fp16 kernel 8 (20 tokens) / 32 (5 tokens), f32 MFMA kernel
4 / 16; row counts 1, V, V + 1, 3 V - 1 (one ragged group, one full, full + ragged, three groups with a ragged last) -- 95 rows at most.

Error measure: err = |got - want| / (|want| + rms(want)) per element.  Bound = 4 x yardstick, the yardstick computed IN the test on the
CPU: the max err of lpbox_hip.policy.EarlyFixPolicy(device="cpu").encode in the kernel's number format (float32 / float16) against the
restatement on the same inputs -- never a figure taken from a kernel.  4: the kernels sum in another order and use the hardware exp
and rcp; the maximum over ~1e5 elements moves by a small factor between orders.  The observed ratios are in
profiles/policy_elements_gpu_tests.txt.

Kernel mutants (each built in a scratch copy of the library, never committed) and the test that fails on each are listed in
DESIGN.md section 20."""
import functools

import numpy as np
import pytest
import torch

from lpbox_hip import policy as P
from lpbox_hip.l2f import fix_vector_from_scores
from oracle import policy_numpy as N
from policy_cases import MARGIN, STATES, TAGS, decisive_input, decisive_scores64, rel_err, state

pytestmark = pytest.mark.gpu

V16 = {20: 8, 5: 32}          # variables per workgroup of policy_body_kernel (160 tokens)
V32 = {20: 4, 5: 16}          # ... of policy_body_f32_kernel8 (80 tokens)
MAX_ROWS = 95
BASE = 3                      # odd offset of the first window in the iterate buffer


def row_counts(v):
    return (1, v, v + 1, 3 * v - 1)


@functools.lru_cache(maxsize=None)
def fused16(name, tokens):
    return P.FusedEarlyFixPolicy(state(name, tokens), tokens=tokens, device="cuda", decision_band=0)


@functools.lru_cache(maxsize=None)
def mfma32(name, tokens):
    return P.MfmaFp32Policy(state(name, tokens), tokens=tokens, device="cuda")


@functools.lru_cache(maxsize=None)
def hip32(name, tokens):
    return P.HipFp32Policy(state(name, tokens), tokens=tokens, device="cuda")


def windows(rows, tokens, stride, seed):
    """An fp64 iterate buffer with one window of (tokens - 1) * stride + 5 values per row, the windows in permuted order behind an odd
    offset, every third row at 0 / 1.  Returns (flat, row_off) as numpy arrays."""
    rs = np.random.RandomState(seed)
    span = (tokens - 1) * stride + 5
    flat = rs.rand(BASE + rows * span + 2)
    row_off = BASE + rs.permutation(rows).astype(np.int64) * span
    for r in range(0, rows, 3):
        flat[row_off[r]:row_off[r] + span] = np.round(flat[row_off[r]:row_off[r] + span])
    return flat, row_off


def dev(flat, row_off):
    return torch.from_numpy(flat).cuda(), torch.from_numpy(row_off).cuda()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# a. per element against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [5, 1, 7])
@pytest.mark.parametrize("name", STATES)
@pytest.mark.parametrize("tokens", [20, 5])
def test_encoder_elements_match_restatement(tokens, name, stride):
    """MfmaFp32Policy.encode and FusedEarlyFixPolicy.encode per element, HipFp32Policy through its logits; token stride 5 (disjoint
    tokens), 1 (overlapping windows: token t = iterates t .. t + 4) and 7 (gaps); rows in permuted order from an odd offset."""
    flat, row_off = windows(MAX_ROWS, tokens, stride, 100 * tokens + stride)
    x = N.tokens_from_flat(flat, row_off, stride, tokens)
    enc64, logit64, _ = N.forward(state(name, tokens), x)
    xt = torch.from_numpy(x)
    cpu32 = P.EarlyFixPolicy(state(name, tokens), tokens=tokens, device="cpu", dtype=torch.float32)
    cpu16 = P.EarlyFixPolicy(state(name, tokens), tokens=tokens, device="cpu", dtype=torch.float16)
    yard = {"f32": cpu32.encode(xt).numpy(), "f16": cpu16.encode(xt).float().numpy()}
    fd, od = dev(flat, row_off)
    tag = "%s %s stride %d" % (TAGS[tokens], name, stride)
    failures = []
    for kind, pol, v in (("f32", mfma32(name, tokens), V32[tokens]), ("f16", fused16(name, tokens), V16[tokens])):
        for n in row_counts(v):
            got = pol.encode(fd, od[:n].contiguous(), stride)
            assert tuple(got.shape) == (n, tokens * 128) and got.dtype == (torch.float32 if kind == "f32" else torch.float16)
            got = got.float().cpu().numpy()
            assert np.isfinite(got).all(), "%s rows %d: non-finite encoder output" % (kind, n)
            y = rel_err(yard[kind][:n], enc64[:n]).max()
            e = rel_err(got, enc64[:n]).max()
            print("RATIO encode_%s %s rows %d: err %.3g yardstick %.3g ratio %.2f" % (kind, tag, n, e, y, e / y))
            if not e < MARGIN * y:
                failures.append((kind, n, float(e), float(y)))
    y = rel_err(cpu32.logits(xt).numpy(), logit64).max()
    _, lg = hip32(name, tokens).scores_from_xiters(fd, od, stride, logits=True)
    e = rel_err(lg.cpu().numpy(), logit64).max()
    print("RATIO score_f32 %s rows %d: logit err %.3g yardstick %.3g ratio %.2f" % (tag, MAX_ROWS, e, y, e / y))
    if not e < MARGIN * y:
        failures.append(("hip32 logit", MAX_ROWS, float(e), float(y)))
    assert not failures, "(kernel, rows, err, yardstick) beyond %g x yardstick: %s" % (MARGIN, failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. isolation, c. ragged tail: bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
ENCODERS = [("f16", 20), ("f16", 5), ("f32", 20), ("f32", 5)]


def encoder(kind, tokens):
    return (fused16("random", tokens), V16[tokens]) if kind == "f16" else (mfma32("random", tokens), V32[tokens])


@pytest.mark.parametrize("kind,tokens", ENCODERS)
def test_variables_of_a_workgroup_do_not_see_each_other(kind, tokens):
    """A full workgroup plus a ragged one.  Replacing the odd-indexed variables' iterates leaves every bit of the even-indexed
    variables' outputs as it was, and the other way round: a key that belongs to the neighbour (the 32-key score tile of the fp16
    kernel spans 1.6 variables of 20 tokens, 6.4 of 5), a query or value row read across the variable's edge would show here."""
    pol, v = encoder(kind, tokens)
    n = v + v // 2 + 1
    rs = np.random.RandomState(7 + tokens)
    x = rs.rand(n, tokens * 5)
    off = torch.arange(n, device="cuda", dtype=torch.int64) * (tokens * 5)
    base = pol.encode(torch.from_numpy(x).cuda().reshape(-1), off, 5)
    for keep in (0, 1):
        x2 = x.copy()
        x2[1 - keep::2] = rs.rand(*x2[1 - keep::2].shape)
        got = pol.encode(torch.from_numpy(x2).cuda().reshape(-1), off, 5)
        assert np.array_equal(bits(got[keep::2]), bits(base[keep::2])), "kept variables (parity %d) changed" % keep
        assert not np.array_equal(bits(got[1 - keep::2]), bits(base[1 - keep::2]))        # the replaced ones did change


@pytest.mark.parametrize("kind,tokens", ENCODERS)
def test_ragged_last_workgroup_gives_the_same_bits_as_a_full_one(kind, tokens):
    """The rows of a last, partial workgroup must not depend on the rows that are missing: appending rows that fill the group
    leaves their bits unchanged (and the first, full group's)."""
    pol, v = encoder(kind, tokens)
    rs = np.random.RandomState(11 + tokens)
    flat = torch.from_numpy(rs.rand(2 * v * tokens * 5)).cuda()
    off = torch.arange(2 * v, device="cuda", dtype=torch.int64) * (tokens * 5)
    full = pol.encode(flat, off, 5)
    for n in (v + 1, 2 * v - 1, 1):
        part = pol.encode(flat, off[:n].contiguous(), 5)
        assert np.array_equal(bits(part), bits(full[:n])), "rows %d" % n


# ---------------------------------------------------------------------------------------------------------------------------------
# d. no write past `rows`
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tokens", ENCODERS)
def test_encoder_writes_nothing_past_rows(kind, tokens):
    """lpbox_policy_encode_f16 / _f32 through the C-ABI with an output buffer one workgroup longer than needed, prefilled with a
    sentinel bit pattern: everything from rows * tokens * 128 on is untouched, the part before it is the encoder output; rows = 0
    returns LPBOX_OK and writes nothing."""
    from lpbox_hip import _lib
    L = _lib.load()
    pol, v = encoder(kind, tokens)
    fn, idt, sentinel = (L.lpbox_policy_encode_f16, torch.int16, 0x5A5A) if kind == "f16" else (L.lpbox_policy_encode_f32, torch.int32, 0x5A5A5A5A)
    rs = np.random.RandomState(13 + tokens)
    width = tokens * 128
    for n in (0, 1, v + 1, 3 * v - 1):
        flat = torch.from_numpy(rs.rand(max(n, 1) * tokens * 5)).cuda()
        off = torch.arange(max(n, 1), device="cuda", dtype=torch.int64) * (tokens * 5)
        out = torch.full(((n + v) * width,), sentinel, dtype=idt, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        rc = fn(flat.data_ptr(), off.data_ptr(), n, tokens, 5, pol.w.data_ptr(), pol.c.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, (n, rc)
        got = out.cpu().numpy()
        assert (got[n * width:] == sentinel).all(), "rows %d: wrote past the end" % n
        if n:
            assert np.array_equal(got[:n * width].reshape(n, width), bits(pol.encode(flat, off[:n].contiguous(), 5)))


# ---------------------------------------------------------------------------------------------------------------------------------
# e. re-score selection, exact
# ---------------------------------------------------------------------------------------------------------------------------------
def band_select(sig, band, thresholds):
    """The kernel's own expression in numpy float32: fabsf(sc - thr_hi) < band || fabsf(sc - thr_lo) < band."""
    sig = np.asarray(sig, np.float32)
    b, hi, lo = np.float32(band), np.float32(thresholds[0]), np.float32(thresholds[1])
    return (np.abs(sig - hi) < b) | (np.abs(sig - lo) < b)


def edge_scores(band, thresholds):
    """float32 scores at thr +- band and at the threshold itself, each with its two float32 neighbours."""
    b32, edge = np.float32(band), []
    for t in (np.float32(thresholds[0]), np.float32(thresholds[1])):
        for e in (t + b32, t - b32, t):
            edge += [e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))]
    return np.array(edge, np.float32)


def test_rescore_band_selects_exactly_the_rows_in_the_band():
    """HipFp32Policy.rescore_band on a hand-made score vector of 2048 + 64 rows (the selection kernel's grid is 2048 workgroups, so
    64 of them take a second variable), 5 tokens: scores at thr +- band and one float32 ulp inside / outside it, at both thresholds,
    the rest anywhere in [0, 1]; for the default band 3e-2 and for 2^-5, where thr +- band is exact in float32 so that
    |score - thr| == band does occur (with 3e-2 no float32 score has that distance: `<` and `<=` would select the same rows).  Selected
    rows become the fp32 score bit for bit, all others keep their bits, the counter grows by the number selected and accumulates over
    a second call.  Then band = 1: every row is selected, the result is the fp32 score of all 2112 rows bit for bit -- the
    grid-stride loop and the reuse of the LDS buffers between its iterations."""
    tokens, rows, thr = 5, 2048 + 64, (0.9, 0.1)
    pol = hip32("random", tokens)
    rs = np.random.RandomState(5)
    flat = torch.from_numpy(rs.rand(rows * 25)).cuda()
    off = (torch.randperm(rows, generator=torch.Generator().manual_seed(6)) * 25).cuda()
    want = pol.scores_from_xiters(flat, off, 5)
    w = want.cpu().numpy()
    base = rs.rand(rows).astype(np.float32)
    base[40:64] = np.float32(0.905)                       # rows 40..63 and their second-iteration partners 2088..2111: both selected
    base[2048 + 40:2048 + 64] = np.float32(0.095)
    for band in (3e-2, 2.0 ** -5):
        sig, edge = base.copy(), edge_scores(band, thr)
        # every edge value twice: once among the first rows, once in the rows that a workgroup reaches in its second iteration
        sig[10:10 + len(edge)] = edge
        sig[2048 + 5:2048 + 5 + len(edge)] = edge
        sel = band_select(sig, band, thr)
        assert 0 < sel.sum() < rows and sel[10:10 + len(edge)].any() and not sel[10:10 + len(edge)].all()
        on_edge = (np.abs(sig - np.float32(thr[0])) == np.float32(band)) | (np.abs(sig - np.float32(thr[1])) == np.float32(band))
        assert not sel[on_edge].any() and (band != 2.0 ** -5 or on_edge.sum() >= 4)      # the distance `band` itself is outside
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        s = torch.from_numpy(sig).cuda()
        pol.rescore_band(flat, off, s, band, thr, 5, counter)
        got = s.cpu().numpy()
        assert np.array_equal(got[sel].view(np.int32), w[sel].view(np.int32)), "band %g: selected rows are not the fp32 scores" % band
        assert np.array_equal(got[~sel].view(np.int32), sig[~sel].view(np.int32)), "band %g: a row outside the band changed" % band
        assert int(counter.item()) == int(sel.sum()), (band, int(counter.item()), int(sel.sum()))
        sel2 = band_select(got, band, thr)                 # second call: the selection now reads the scores the first call left
        pol.rescore_band(flat, off, s, band, thr, 5, counter)
        got2 = s.cpu().numpy()
        assert np.array_equal(got2[sel2].view(np.int32), w[sel2].view(np.int32)) and np.array_equal(got2[~sel2].view(np.int32), got[~sel2].view(np.int32))
        assert int(counter.item()) == int(sel.sum()) + int(sel2.sum())
    s = torch.from_numpy(base).cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    pol.rescore_band(flat, off, s, 1.0, thr, 5, counter)
    assert np.array_equal(bits(s), bits(want)) and int(counter.item()) == rows


# ---------------------------------------------------------------------------------------------------------------------------------
# f. decisions that exist
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [20, 5])
def test_fix_decisions_on_a_decisive_state(tokens):
    """random_state(seed=2) with fc4 scaled by 200 and centred at the median float64 logit: the scores of 3000 rows (1200 at 0 / 1)
    spread over (0, 1) -- restatement: 4.0 % / 13 % above 0.9, 7.1 % / 14 % below 0.1, 271 / 392 rows within 3e-2 of a threshold
    (20 / 5 tokens).  (i) the fused policy's result is the fp32 kernel's score where its fp16 score lies in the band and the fp16
    score elsewhere, bit for bit, and `rescored` counts those rows; (ii) its fix vector is the restatement's, rows within 1e-4 of a
    threshold in float64 left out (30 x the fp32 error of 3e-6 on this sigmoid; at most 0.5 % of the rows); (iii) so are the fix
    vectors of the two fp32 paths."""
    sd, x, s64 = state("decisive", tokens), decisive_input(tokens), decisive_scores64(tokens)
    rows = x.shape[0]
    near64 = np.minimum(np.abs(s64 - 0.9), np.abs(s64 - 0.1))
    # not vacuous, on the restatement alone
    assert (s64 > 0.9).mean() >= 0.03 and (s64 < 0.1).mean() >= 0.03
    assert (near64 < 3e-2).sum() >= 100
    flat = x.to(torch.float64).reshape(-1).cuda()
    off = torch.arange(rows, device="cuda", dtype=torch.int64) * (tokens * 5)
    s16 = P.FusedEarlyFixPolicy(sd, tokens=tokens, device="cuda", decision_band=0).scores_from_xiters(flat, off, 5).cpu().numpy()
    fused = P.FusedEarlyFixPolicy(sd, tokens=tokens, device="cuda")
    h32 = P.HipFp32Policy(sd, tokens=tokens, device="cuda")
    s32 = h32.scores_from_xiters(flat, off, 5).cpu().numpy()
    got = fused.scores_from_xiters(flat, off, 5).cpu().numpy()
    sel = band_select(s16, fused.decision_band, fused.thresholds)
    print("DECISIVE %s: above 0.9 %.3f, below 0.1 %.3f, in band (float64) %d, re-scored %d, max |s16 - s64| %.3g, max |s32 - s64| %.3g"
          % (TAGS[tokens], (s64 > 0.9).mean(), (s64 < 0.1).mean(), (near64 < 3e-2).sum(), sel.sum(), np.abs(s16 - s64).max(), np.abs(s32 - s64).max()))
    assert sel.sum() > 0 and fused.rescored == int(sel.sum())                                        # (i)
    assert np.array_equal(got[sel].view(np.int32), s32[sel].view(np.int32))
    assert np.array_equal(got[~sel].view(np.int32), s16[~sel].view(np.int32))
    clear = near64 >= 1e-4                                                                           # (ii), (iii)
    assert (~clear).sum() <= 0.005 * rows
    want = fix_vector_from_scores(s64)[0]
    m32 = P.MfmaFp32Policy(sd, tokens=tokens, device="cuda").scores_from_xiters(flat, off, 5).cpu().numpy()
    for label, sc in (("fused", got), ("mfma32", m32), ("hip32", s32)):
        vec = fix_vector_from_scores(sc)[0]
        bad = np.nonzero((vec != want) & clear)[0]
        assert bad.size == 0, "%s: %d decisions differ, first rows %s scores %s float64 %s" % (label, bad.size, bad[:5], sc[bad[:5]], s64[bad[:5]])
