"""Mixture of search algorithms (hyperopt/mix.py:5-35).

``suggest`` hands each call to one of several suggest functions, chosen with
the given probabilities:

    fmin(..., algo=partial(mix.suggest, p_suggest=[(.1, rand.suggest),
                                                   (.2, anneal.suggest),
                                                   (.7, tpe.suggest)]))

Same stream as the reference: ``RandomState(seed)``, one multinomial draw for
the choice, then ``randint(2 ** 31)`` for the seed handed down.  Any callable
with the ``(new_ids, domain, trials, seed)`` signature can take part
(rand.suggest, rand.suggest_device, anneal.suggest, tpe.suggest, ...).
"""
from __future__ import annotations

import numpy as np


def suggest(new_ids, domain, trials, seed, p_suggest):
    """The documents of a randomly chosen suggest function.

    p_suggest: list of (probability, suggest) pairs; the probabilities must
    sum to (about) 1, else ValueError."""
    rng = np.random.RandomState(seed)
    ps = [p for p, _ in p_suggest]
    suggests = [s for _, s in p_suggest]
    if not np.isclose(sum(ps), 1.0):
        raise ValueError("Probabilities should sum to 1", tuple(ps))
    idx = int(rng.multinomial(n=1, pvals=ps).argmax())
    return suggests[idx](new_ids, domain, trials, seed=rng.randint(2 ** 31))
