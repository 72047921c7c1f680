"""Spaces of the annealing fixtures, shared by the generator (reference hp) and
the tests (our hp), like spaces.py: one prior of every kind."""

KINDS = ["uniform", "quniform", "loguniform", "qloguniform", "normal", "qnormal", "lognormal",
         "qlognormal", "randint10", "randint12_25", "pchoice"]


def prior(hp, kind, label):
    if kind == "uniform":
        return hp.uniform(label, -3, 4)
    if kind == "quniform":
        return hp.quniform(label, 0, 10, 3)
    if kind == "loguniform":
        return hp.loguniform(label, -2, 1)
    if kind == "qloguniform":
        return hp.qloguniform(label, 0, 3, 2)
    if kind == "normal":
        return hp.normal(label, 1, 2)
    if kind == "qnormal":
        return hp.qnormal(label, 0, 10, 2)
    if kind == "lognormal":
        return hp.lognormal(label, 0.5, 0.7)
    if kind == "qlognormal":
        return hp.qlognormal(label, 0, 1, 0.5)
    if kind == "randint10":
        return hp.randint(label, 10)
    if kind == "randint12_25":
        return hp.randint(label, 12, 25)
    if kind == "pchoice":
        return hp.pchoice(label, [(0.1, 0), (0.3, 1), (0.6, 2)])
    raise KeyError(kind)


def single(hp, kind):
    """One label, "x", of the given kind."""
    return {"x": prior(hp, kind, "x")}


def flat(hp):
    """The eleven kinds in one flat space, each labelled by its kind."""
    return {kind: prior(hp, kind, kind) for kind in KINDS}
