"""GPU path vs the reference's own outputs (golden vectors).

Every case of tests/golden/reference_cases.json — produced by running the
reference's ``activestorage/storage.py`` on the reference's own test inputs
(cesm2/daily_data/zero_chunked byte ranges of tests/unit/test_storage.py,
every chunk of test1.nc with zlib+shuffle, cesm2 chunks) and on a synthetic
sweep — is replayed through the HIP drop-in ``reduce_chunk_bytes``.  Same
container type, dtype, shape, nomask-ness, mask and count; values bit-exact
(a zero min/max down to its sign bit) except float sums/means (float32:
<= 1e-6 relative, cancelling sums within 4e-7 * sum|x|, counted and
reported; float64: within tests/_compare.sum_bound of NumPy's result).
Cases where the reference raises must raise the same exception type.
"""
import numpy as np
import pytest

from pyactivestorage_amd import storage as pas
from tests import _golden as G

pytestmark = pytest.mark.gpu


FALLBACKS = []


@pytest.mark.parametrize("block", range(0, len(G.cases()), 400))
def test_gpu_reproduces_reference_outputs(gpu, block):
    cases = G.cases()
    for i in range(block, min(block + 400, len(cases))):
        a = G.args_of(i, pas.Zlib, pas.Shuffle)
        exp = G.expected(i)
        call = lambda: pas.reduce_chunk_bytes(a["raw"], a["compression"], a["filters"], a["missing"],  # noqa
                                              a["dtype"], a["shape"], a["order"], a["chunk_selection"],
                                              a["axis"], a["method"])
        if isinstance(exp[0], str):
            with pytest.raises(Exception) as ei:
                call()
            assert type(ei.value).__name__ == exp[0], (i, G.cases()[i], ei.value)
            continue
        tmp, n = call()
        if G.check_gpu(i, tmp, n, a, pas.reduce_chunk_bytes):
            FALLBACKS.append(i)


def test_report_cancelling_sum_fallbacks(gpu):
    """How many float sum/mean cases sat outside 1e-6 relative but within
    4e-7 * sum|x| (cancelling sums only; see tests/_golden.py check_gpu)."""
    n_float_sums = sum(1 for c in G.cases() if "raises" not in c and c["dtype"].lstrip("<>=|")[0] == "f"
                       and c["method"] in ("ma.sum", "sum", "ma.mean", "mean"))
    n_zero = sum(1 for i, c in enumerate(G.cases()) if "raises" not in c and c["method"].endswith(("min", "max"))
                 and c["dtype"].lstrip("<>=|")[0] == "f" and (G.expected(i)[1] == 0).any())
    print(f"\ngolden float sum/mean cases: {n_float_sums}; needing the cancelling-sum bound: "
          f"{len(FALLBACKS)} {FALLBACKS}; min/max cases with a zero result: {n_zero}; "
          f"zero sign bits compared: {G.signs_comparable()}; float64 sum/mean cases held to sum_bound: "
          f"{G.F64_STATS['cases']}, worst error/bound {G.F64_STATS['worst']:.3f}")
    assert G.F64_STATS["worst"] <= 1.0
    assert len(FALLBACKS) <= n_float_sums
    if not G.signs_comparable():
        pytest.skip("this host's NumPy breaks zero ties unlike the golden host: zero signs compared by value")
