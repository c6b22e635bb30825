"""ultranest_amd -- MI355X (gfx950) implementation of UltraNest's MLFriends hot path.

Drop-in for ``ultranest.mlfriends`` on that path only: region construction
(bootstrapped ``compute_maxradiussq``), the membership test (``find_nearby`` / ``inside``) and
the vectorized-likelihood batch call.  Compute runs in hand-written HIP kernels behind the C ABI
of ``include/mlfriends_hip.h``; there is no CPU fallback.
"""
__version__ = "0.1.0"

from . import priors  # noqa: E402,F401  (the prior library of device models: ultranest_amd.priors)
from . import hotstart  # noqa: E402,F401  (warm start, auxiliary problems on the host and on the device routes)
