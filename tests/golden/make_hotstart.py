"""Writes tests/golden/g19_hotstart.npz: what the reference's ``ultranest/hotstart.py`` returns for the seeded sample sets and
cube rows of tests/hotstart_reference.py (run from the repository root:
``python tests/golden/make_hotstart.py /path/to/UltraNest``, the directory that holds the reference's ``ultranest`` package).

Only ``ultranest/hotstart.py`` and ``ultranest/utils.py`` of the reference are executed (through a stub package, so its
compiled modules are not needed); the fixture holds numbers only.  Keys, per d in (1, 2, 5) and n in (11, 400), prefix
``d<d>_n<n>_``: upoints, uweights, ulos, uhis, uinterpspace; ``box_u`` / ``box_p`` / ``box_L`` the contbox rows, transform
rows and likelihoods; ``ind_u`` / ``ind_p`` / ``ind_L``, ``rot_u`` / ``rot_p`` / ``rot_L`` and ``ext_u`` / ``ext_p`` / ``ext_L``
the same for the independent, rotated and extended rotated Student-t problems (df = 1 for n = 11, df = 4.5 for n = 400)."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hotstart_reference as HR  # noqa: E402


def reference_hotstart(root):
    pkg = types.ModuleType("ultranest")
    pkg.__path__ = [os.path.join(root, "ultranest")]
    sys.modules["ultranest"] = pkg
    return importlib.import_module("ultranest.hotstart")


def df_of(n):
    return 1 if n == 11 else 4.5


def main():
    ref = reference_hotstart(sys.argv[1])
    arrays = {}
    for d in HR.DIMS:
        for n in HR.NSAMPLES:
            key = "d%d_n%d_" % (d, n)
            up, w = HR.samples(d, n)
            ulos, uhis, xp = ref.compute_quantile_intervals_refined(HR.STEPS, up, w)
            arrays.update({key + "upoints": up, key + "uweights": w, key + "ulos": ulos, key + "uhis": uhis, key + "uinterpspace": xp})
            names, L, T, vec = ref.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], HR.host_loglike, HR.host_transform,
                                                                           up, w, vectorized=True)
            u = HR.contbox_test_rows(d, xp, seed=d + n)
            p = T(u)
            arrays.update({key + "box_u": u, key + "box_p": p, key + "box_L": L(p)})
            L1, T1 = ref.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], HR.host_loglike, HR.host_transform, up, w)[1:3]
            assert np.array_equal(np.array([T1(row) for row in u]), p, equal_nan=True)
            ctr, err, invcov = HR.moments(up, w)
            df = df_of(n)
            u = HR.cube_test_rows(d, seed=7 * d + n)
            with np.errstate(all="ignore"):
                L, T = ref.get_extended_auxiliary_independent_problem(HR.host_loglike, HR.host_transform, ctr, err, df=df)
                p = np.array([T(row) for row in u])
                arrays.update({key + "ind_u": u, key + "ind_p": p, key + "ind_L": np.array([L(row) for row in p])})
                L, T = ref.get_auxiliary_problem(HR.host_loglike, HR.host_transform, ctr, invcov, np.sqrt(d), df=df)
                arrays.update({key + "rot_u": u, key + "rot_p": np.array([T(row) for row in u]), key + "rot_L": np.array([L(row) for row in u])})
                L, T = ref.get_extended_auxiliary_problem(HR.host_loglike, HR.host_transform, ctr, invcov, np.sqrt(d), df=df)
                p = np.array([T(row) for row in u])
                arrays.update({key + "ext_u": u, key + "ext_p": p, key + "ext_L": np.array([L(row) for row in p])})
    np.savez_compressed(HR.FIXTURE, **arrays)
    print(HR.FIXTURE, os.path.getsize(HR.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
