"""The space and the case the liar-chain tests share (CPU and GPU)."""
import numpy as np

from hyperopt_amd import Domain, hp, rand, tpe
from tests import joint_util as U


def chain_space():
    """A root of three labels; ``w`` reachable from two branches (its context keeps
    the selector ``s``); ``z`` / ``zz`` nested; every factor kind on both sides of a
    boundary: contexts hold r (continuous), rq (quantized), s (discrete)."""
    w = hp.uniform("w", 0, 1)
    inner = hp.choice("t", [{"z": hp.quniform("z", 0, 8, 2)}, {"zz": hp.randint("zz", 3)}])
    return {"r": hp.loguniform("r", -2, 1), "rq": hp.quniform("rq", 0, 8, 2),
            "s": hp.choice("s", [
                {"w": w, "q": hp.qlognormal("q", 0, 1, 0.5), "n": hp.normal("n", 0, 1),
                 "c": hp.pchoice("c", [(0.3, 0), (0.7, 1)])},
                {"w": w, "inner": inner}, {"lone": hp.uniform("lone", 0, 1)}])}


def chain_case(P, seed, space=chain_space):
    """(domain, 40 trials, pool of P rows); branch 2 of ``s`` is in no trial and no row."""
    rng = np.random.RandomState(seed)
    domain = Domain(lambda x: 0, space())
    cfgs = [c for c in (rand.sample_config(domain, rng) for _ in range(3 * P + 320))
            if c.get("s") != 2]
    return domain, U.make_trials(domain, cfgs[:40], rng.uniform(size=40)), \
        tpe.Pool(domain, cfgs[40:40 + P])
