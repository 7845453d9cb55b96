"""CPU tests: the float64 numpy restatement of the policy network (oracle/policy_numpy.py, written from the reference's mha.py and
position code alone) pinned to the reference module's own outputs, and lpbox_hip/policy.py's folded evaluation pinned to the
restatement PER ELEMENT of the encoder output -- the quantity the HIP encoder kernels produce (tests/test_policy_elements_gpu.py).

Error measure everywhere: err = |got - want| / (|want| + rms(want)), element-wise, maximum over the array.

Yardstick: the reference module evaluates in float32; its own outputs (tests/golden/policy_encoder_reference.npz, made by
make_policy_encoder_fixture.py from the reference module, and the older policy_reference.npz) differ from the float64 restatement
by the figures in REF_ERR below, measured once on the CPU.  Every bound is 4 x such a figure: torch's CPU GEMM blocking may differ
between builds, which moves a float32 maximum by a small factor, while every defect of the restatement or of the folding that the
mutants below stand for moves it by four orders of magnitude or more.

Mutants of the restatement (made in a scratch copy, not committed), err of the reference's lp / seg encoder output against them:
(stress: lp, seg; random: lp, seg), all in test_restatement_matches_reference_module:
  head order swapped in W_out (wo[7 - h])       0.71, 0.72; 2.2, 2.3           caught in all four cases
  position row 0 not zeroed                     unchanged: 0 / 10000^p is 0 already, so sin / cos give the same row 0,1,0,1,0 -- an
                                                equivalent mutant, nothing can catch it.  Its live neighbour, zeroing row 0 AFTER
                                                sin / cos (row 0 = 0,0,0,0,0):  1.3e-2, 3.2e-2; 0.87, 0.96   caught in all four cases
  BN eps dropped                                2.1e-5, 2.0e-5; 1.5e-5, 1.5e-5  caught on "random" (5.0 x and 4.4 x the bound) and on
                                                lp stress (1.1 x); seg stress alone would miss it (0.9 x)
  softmax without the 1/4 scale                 9.5e-3, 1.3e-2; 0.64, 0.86     caught in all four cases
  residual before the BN, not after it          0.45, 0.45; 1.1e-5, 1.1e-5     caught in all four cases (random: 3.8 x, 3.1 x the bound;
                                                the random state's BatchNorm is nearly the identity)"""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from lpbox_hip import policy as P
from oracle import policy_numpy as N
from policy_cases import ENC_FIX, MARGIN, STATES, TAGS, rel_err, rounded_input, state

OLD_FIX = np.load(os.path.join(GOLDEN, "policy_reference.npz"))

# max err of the reference module's float32 output against the restatement (measured on the CPU, torch 2.x, one thread or many)
REF_ERR = {
    ("lp", "stress"): {"encoder": 4.86e-6, "logit": 6.03e-6},
    ("lp", "random"): {"encoder": 7.53e-7, "logit": 3.24e-7},
    ("seg", "stress"): {"encoder": 5.38e-6, "logit": 3.70e-5},
    ("seg", "random"): {"encoder": 8.74e-7, "logit": 3.15e-7},
}
OLD_REF_ERR = {"lp": 1.98e-5, "seg": 2.77e-5}      # the 96 logits of policy_reference.npz (stress weights)


@pytest.mark.parametrize("name", STATES)
@pytest.mark.parametrize("tokens", [20, 5])
def test_restatement_matches_reference_module(tokens, name):
    """Encoder output per element, logit and sigmoid of the restatement against the reference module's (8 rows, 3 of them at 0 / 1).
    Measured max err of the reference's float32 against the restatement: encoder 4.86e-6 (lp stress), 5.38e-6 (seg stress), 7.53e-7
    (lp random), 8.74e-7 (seg random); logit 6.03e-6, 3.70e-5, 3.24e-7, 3.15e-7.  Bound: 4 x each."""
    tag = TAGS[tokens]
    key = "%s_%s_" % (tag, name)
    enc, logit, sig = N.forward(state(name, tokens), ENC_FIX[key + "x"])
    assert enc.shape == ENC_FIX[key + "encoder"].shape and enc.dtype == np.float64
    e_enc, e_lg = rel_err(ENC_FIX[key + "encoder"], enc).max(), rel_err(ENC_FIX[key + "logit"], logit).max()
    print("%s %s: reference fp32 vs restatement: encoder err %.3g, logit err %.3g" % (tag, name, e_enc, e_lg))
    assert e_enc < MARGIN * REF_ERR[tag, name]["encoder"]
    assert e_lg < MARGIN * REF_ERR[tag, name]["logit"]
    # the sigmoid is 1 / (1 + exp(-logit)): its slope is at most 1/4, so the logit bound carries over in absolute terms
    lg_abs = MARGIN * REF_ERR[tag, name]["logit"] * (np.abs(logit).max() + np.sqrt(np.mean(logit * logit)))
    assert np.abs(ENC_FIX[key + "sigmoid"] - sig).max() < 0.25 * lg_abs + 6e-8      # + half a float32 ulp of a value below 1


@pytest.mark.parametrize("tokens", [20, 5])
def test_restatement_matches_the_first_golden_logits(tokens):
    """The 96 rows of policy_reference.npz (stress weights), which tests/test_policy.py compares the kernels' sigmoid with.
    Measured max err of the reference's float32 logits against the restatement: 1.98e-5 (lp), 2.77e-5 (seg).  Bound: 4 x each."""
    tag = TAGS[tokens]
    _, logit, sig = N.forward(state("stress", tokens), OLD_FIX[tag + "_x"])
    e = rel_err(OLD_FIX[tag + "_logit"], logit).max()
    print("%s: golden logits vs restatement: err %.3g" % (tag, e))
    assert e < MARGIN * OLD_REF_ERR[tag]
    assert np.abs(OLD_FIX[tag + "_sigmoid"] - sig).max() < 0.25 * MARGIN * OLD_REF_ERR[tag] * 2 * np.abs(logit).max() + 6e-8


@pytest.mark.parametrize("name", STATES)
@pytest.mark.parametrize("tokens", [20, 5])
def test_folded_policy_encoder_matches_restatement(tokens, name):
    """EarlyFixPolicy.encode (position code folded into a bias, Q|K|V of all heads in one matrix, W_out reshaped, BatchNorm folded to
    scale / shift) in float32 on the CPU, per element against the restatement: 67 rows in two chunks, the first 20 at 0 / 1.  Bound:
    4 x the reference module's own float32 error in the same state (REF_ERR): the folding is the same arithmetic in another order."""
    x = rounded_input(67, tokens, 20, 3)
    enc, logit, _ = N.forward(state(name, tokens), x.numpy())
    pol = P.EarlyFixPolicy(state(name, tokens), tokens=tokens, device="cpu", chunk_rows=40)
    got = pol.encode(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (67, tokens * 128)
    e = rel_err(got.numpy(), enc).max()
    print("%s %s: EarlyFixPolicy.encode fp32 vs restatement: err %.3g" % (TAGS[tokens], name, e))
    assert e < MARGIN * REF_ERR[TAGS[tokens], name]["encoder"]
    # the split left the scores what they were: head(encode(x)) is logits(x), bit for bit
    z = got
    for k, (w, b) in enumerate(pol.head):
        z = z @ w + b
        if k < 3:
            z = torch.relu(z)
    assert torch.equal(z.view(-1)[:40], pol.logits(x)[:40])


def test_tokens_from_flat_reads_like_the_kernels():
    """token t of row r = flat[row_off[r] + t * tok_stride : + 5], for disjoint, overlapping and gapped tokens."""
    flat = np.arange(200, dtype=np.float64)
    for stride in (5, 1, 7):
        x = N.tokens_from_flat(flat, [3, 50, 0], stride, 5)
        assert x.shape == (3, 5, 5)
        for r, off in enumerate((3, 50, 0)):
            for t in range(5):
                assert x[r, t].tolist() == flat[off + t * stride: off + t * stride + 5].tolist()
    assert N.position_code(20)[0].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
