"""Shared by tests/test_policy_restatement.py and tests/test_policy_elements_gpu.py: the weight states, the inputs and the error
measure of the policy tests, with the float64 restatement (oracle/policy_numpy.py) computed once per case."""
import functools
import os
import sys

import numpy as np
import torch

from helpers import GOLDEN
from lpbox_hip import policy as P
from oracle import policy_numpy as N

sys.path.insert(0, GOLDEN)
from make_policy_fixture import deterministic_state  # noqa: E402

ENC_FIX = np.load(os.path.join(GOLDEN, "policy_encoder_reference.npz"))
TAGS = {20: "lp", 5: "seg"}
STATES = ("stress", "random")
MARGIN = 4.0          # bound = MARGIN x yardstick (another summation order moves the maximum over ~1e5 elements by a small factor)

rel_err = N.rel_err


@functools.lru_cache(maxsize=None)
def state(name, tokens):
    """"stress": weights by formula (make_policy_fixture.deterministic_state); "random": drawn like the reference initialises them;
    "decisive": random_state(seed=2) with the last layer scaled by 200 and centred, so that the scores spread over (0, 1)."""
    if name == "stress":
        return deterministic_state(P.reference_state_shapes(tokens))
    if name == "random":
        return P.random_state(tokens, seed=5)
    if name == "decisive":
        sd, _, logit = _decisive_base(tokens)
        sd = dict(sd)
        sd["classify.fc4.weight"] = sd["classify.fc4.weight"] * 200.0
        sd["classify.fc4.bias"] = sd["classify.fc4.bias"] * 200.0 - torch.tensor([200.0 * float(np.median(logit))], dtype=torch.float32)
        return sd
    raise ValueError(name)


def rounded_input(rows, tokens, n_rounded, seed):
    """float32 (rows, tokens, 5), uniform in [0, 1], the first n_rounded rows at 0 / 1 (converged iterates)."""
    x = torch.rand(rows, tokens, 5, generator=torch.Generator().manual_seed(seed))
    x[:n_rounded] = torch.round(x[:n_rounded])
    return x


@functools.lru_cache(maxsize=None)
def decisive_input(tokens):
    return rounded_input(3000, tokens, 1200, 7)


@functools.lru_cache(maxsize=None)
def _decisive_base(tokens):
    """The unscaled state, and the restatement's encoder output and logits of it on the decisive input (the scaling touches fc4 only)."""
    sd = P.random_state(tokens, seed=2)
    enc, logit, _ = N.forward(sd, decisive_input(tokens).numpy())
    return sd, enc, logit


@functools.lru_cache(maxsize=None)
def decisive_scores64(tokens):
    """float64 scores of the decisive state on the decisive input."""
    return N.head(state("decisive", tokens), _decisive_base(tokens)[1])[1]
