"""Writes tests/golden/g17_special_priors.npz: the 60-digit mpmath quantiles of tests/special_prior_reference.py for every
setting of its SETTINGS table on its grid (run from the repository root: python tests/golden/make_special_priors.py).
Nothing but this repository's own mpmath code is read."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import special_prior_reference as SR  # noqa: E402
from ultranest_amd import priors as P  # noqa: E402


def main():
    arrays = {}
    for family in SR.FAMILY_NAMES:
        for name in SR.settings(family):
            t0 = time.time()
            prior = SR.SETTINGS[name]()
            u = SR.block_grid(prior.size) if isinstance(prior, P.Dirichlet) else SR.grid()
            arrays.update(SR.pack(name, prior, u, SR.reference(prior, u)))
            print("%-16s %4d values  %.1f s" % (name, np.size(u), time.time() - t0), flush=True)
    np.savez_compressed(SR.FIXTURE, **arrays)
    print(SR.FIXTURE, os.path.getsize(SR.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
