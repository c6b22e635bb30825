#!/usr/bin/env python3
"""Records tests/golden/g18_prior_sources.json: the sha256 of ``PriorTransform(...).source`` for a fixed set of lists that hold
neither a ``Ref`` nor a ``Tabulated``.  The file was written at the commit before those two existed; a list of constant
priors must keep producing exactly that text, so that every cache key and code object derived from it stays what it was
(tests/test_prior_rt_compile.py compares).

    python tests/golden/make_prior_sources.py [--out tests/golden/g18_prior_sources.json]

Needs no GPU and compiles nothing: ``source`` is text.
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def lists():
    """{name: list of priors}: the mixed list of test_priors_compile, one list per closed-form family (its three settings),
    both blocks, one list with iterative families and one with the Dirichlet block"""
    import numpy as np
    import prior_reference as PR
    from test_priors_compile import mixed_priors
    from ultranest_amd import priors as P
    out = {"mixed12": mixed_priors()}
    for name in sorted(PR.FAMILIES):
        out["family_" + name] = PR.family(name)
    A = np.random.RandomState(8).normal(size=(8, 8))
    cov = A.dot(A.T) + 8 * np.eye(8)
    out["block_mvn8"] = [P.MultivariateNormal(np.arange(8), 0.5 * (cov + cov.T))]
    out["block_ordered5"] = [P.OrderedUniform(-1.0, 3.0, 5)]
    out["iterative"] = [P.Normal(0.0, 1.0), P.Gamma(2.5, 3.0), P.ChiSquared(4.0), P.InverseGamma(3.0, 2.0), P.Beta(0.5, 2.0),
                        P.StudentT(3.0, 1.0, 2.0)]
    out["dirichlet3"] = [P.Dirichlet([0.5, 1.0, 2.0]), P.Uniform(0.0, 1.0)]
    return out


def hashes():
    from ultranest_amd import priors as P
    return {name: hashlib.sha256(P.PriorTransform(pri).source.encode()).hexdigest() for name, pri in sorted(lists().items())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "g18_prior_sources.json"))
    args = ap.parse_args()
    with open(args.out, "w") as fh:
        json.dump(hashes(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %d hashes to %s" % (len(hashes()), args.out))
