"""GPU parity: fft / ifft / coset_fft / coset_ifft (src/fft.rs:160-198) through the C-ABI vs the oracle
and the committed golden vectors.  Bit-exact."""
import numpy as np
import pytest

from conftest import golden, h2i

pytestmark = pytest.mark.gpu
FNS = ("fft", "ifft", "coset_fft", "coset_ifft")


def _rand(O, n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 60) - 1)
    return O.to_mont(O.FR, raw)


def test_fft_simple_input_kat(srs, oracle):
    """src/fft.rs:241-260 through the GPU path."""
    O = oracle
    kat = golden("kat.json")["fft_simple_input_test"]
    a = O.ints_to_mont(O.FR, kat["input"])
    assert [str(v) for v in O.mont_to_ints(O.FR, srs.fft.fft(a))] == kat["output"]


def test_ntt_golden(srs, oracle):
    O = oracle
    for rec in golden("ntt.json"):
        a = O.ints_to_mont(O.FR, [h2i(x) for x in rec["input"]])
        for fn in FNS:
            got = O.mont_to_ints(O.FR, getattr(srs.fft, fn)(a.copy()))
            assert got == [h2i(x) for x in rec[fn]], (rec["k"], fn)


@pytest.mark.parametrize("k", [0, 1, 4, 5, 8, 10, 11, 12, 13, 16, 17, 18, 20])
def test_ntt_vs_oracle(srs, oracle, k):
    """k=4..8: reference's fft_random_input_test sizes (src/fft.rs:268-296); 11+ exercise the multi-pass path;
    sizes of the real path (32, 8, 256 points) are k=5, 3 (golden), 8."""
    O = oracle
    a = _rand(O, 1 << k, 100 + k)
    for fn in FNS:
        assert np.array_equal(getattr(srs.fft, fn)(a.copy()), getattr(O, fn)(a)), (k, fn)


@pytest.mark.parametrize("k", [6, 14, 19])
def test_roundtrips_device_resident(srs, oracle, k):
    """fft∘ifft = id and coset_fft∘coset_ifft = id (src/fft.rs:268-296) on device-resident data."""
    import torch
    O = oracle
    a = _rand(O, 1 << k, 7 + k)
    d = torch.from_numpy(a.view(np.int64)).cuda()
    srs.fft.fft(d); srs.fft.ifft(d)
    assert np.array_equal(d.cpu().numpy().view(np.uint64), a)
    srs.fft.coset_fft(d); srs.fft.coset_ifft(d)
    assert np.array_equal(d.cpu().numpy().view(np.uint64), a)


def test_ntt_pass_structures(srs, oracle):
    """Every digit split (2, 3 and 4 passes) gives the same bits."""
    from sirius_amd import _lib
    O = oracle
    try:
        for bits, k in ((4, 12), (4, 16), (5, 15), (6, 17), (7, 21)):
            assert _lib.lib().srs_ntt_set_max_radix_bits(bits) == bits
            a = _rand(O, 1 << k, bits * 100 + k)
            assert np.array_equal(srs.fft.fft(a.copy()), O.fft(a)), (bits, k)
            assert np.array_equal(srs.fft.coset_ifft(a.copy()), O.coset_ifft(a)), (bits, k)
    finally:
        _lib.lib().srs_ntt_set_max_radix_bits(8)


def _extreme_inputs(O, k, seed):
    """Canonical Montgomery words that drive the lazy tile to its bounds: p - 1 is the largest admissible bit pattern."""
    from oracle import pyref as P
    n = 1 << k
    pm1 = np.array([[((P.MODULI[0] - 1) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]], dtype=np.uint64)
    one = O.ints_to_mont(O.FR, [1])                        # the field's 1 (R mod p as a word)
    zero = np.zeros((n, 4), np.uint64)
    alt = _rand(O, n, seed)
    alt[::2] = pm1
    first, last, lead = zero.copy(), zero.copy(), zero.copy()
    first[0], last[n - 1], lead[0] = one, one, pm1
    return {"all p - 1": np.repeat(pm1, n, axis=0), "p - 1 / random": alt, "all zero": zero, "1 at 0": first, "1 at n - 1": last,
            "(p - 1, 0, 0, ...)": lead}


# max radix bits -> size, as in test_ntt_pass_structures: 2, 3 and 4 passes
_SPLITS = {12: (4,), 16: (4,), 15: (5,), 17: (6,), 21: (7,)}


@pytest.mark.parametrize("k", [8, 11, 12, 15, 16, 17, 20, 21])
def test_ntt_lazy_tile_extremes(srs, oracle, k):
    """The GPU twin of test_emu_ntt_lazy_tile_extremes: the real kernels on the inputs that push the lazy 9 x 29-bit tile to its limits -- every
    element p - 1, alternating p - 1 / random, all zero, a single 1 at either end, (p - 1, 0, 0, ...) -- all four transforms, bit-exact
    against the oracle; at the default radix and, at the sizes test_ntt_pass_structures uses for 2, 3 and 4 passes, with the digit width
    limited to 4 .. 7 bits (each oracle result is computed once and serves both).  The words are canonical Montgomery words as everywhere
    in this file: the tile derives its bounds from "canonical input" (csrc/ntt.hip), so p - 1 everywhere is the worst ADMISSIBLE input
    and non-canonical words are outside the contract -- they are not fed."""
    from sirius_amd import _lib
    O = oracle
    try:
        for name, a in _extreme_inputs(O, k, 300 + k).items():
            want = {fn: getattr(O, fn)(a) for fn in FNS}
            for bits in (8,) + _SPLITS.get(k, ()):
                assert _lib.lib().srs_ntt_set_max_radix_bits(bits) == bits
                for fn in FNS:
                    assert np.array_equal(getattr(srs.fft, fn)(a.copy()), want[fn]), (k, name, fn, bits)
    finally:
        _lib.lib().srs_ntt_set_max_radix_bits(8)


def test_ntt_microbench_size_properties(srs, oracle):
    """BASELINE config 5 size (2^24), too slow for the oracle in a unit test: size-independent properties --
    round trip, linearity against a second vector, and a spot check of one output against the definition."""
    import torch
    O = oracle
    k = 24
    n = 1 << k
    a, b = _rand(O, n, 1), _rand(O, n, 2)
    da = torch.from_numpy(a.view(np.int64)).cuda()
    db = torch.from_numpy(b.view(np.int64)).cuda()
    dab = torch.from_numpy(O.fe_add(O.FR, a, b).view(np.int64)).cuda()
    srs.fft.fft(da); srs.fft.fft(db); srs.fft.fft(dab)
    fa, fb, fab = (t.cpu().numpy().view(np.uint64) for t in (da, db, dab))
    assert np.array_equal(O.fe_add(O.FR, fa, fb), fab)                     # linearity
    # X[0] = sum a_i, X[n/2] = sum (-1)^i a_i  (definition of the DFT at w^0 and w^(n/2) = -1)
    ints = np.array(O.mont_to_ints(O.FR, a[: 1 << 12]), dtype=object)       # cheap partial check on a chunk is meaningless;
    del ints                                                                # use full sums via the oracle field adds instead
    s = a.copy()
    while s.shape[0] > 1:
        h = s.shape[0] // 2
        s = O.fe_add(O.FR, s[:h], s[h:])
    assert np.array_equal(fa[0], s[0])
    alt = a.copy()
    alt[1::2] = O.fe_sub(O.FR, np.zeros_like(alt[1::2]), alt[1::2])
    while alt.shape[0] > 1:
        h = alt.shape[0] // 2
        alt = O.fe_add(O.FR, alt[:h], alt[h:])
    assert np.array_equal(fa[n // 2], alt[0])
    srs.fft.ifft(da)
    assert np.array_equal(da.cpu().numpy().view(np.uint64), a)             # round trip


def test_ntt_config_2p24_vs_oracle(srs, oracle):
    """BASELINE configs[4]: the 2^24-point transforms compared DIRECTLY with the oracle's restatement of src/fft.rs:160-198 (three passes of
    2^8: a digit-reversal slip that only shows with three digits would pass every size-independent property but not this).  The OpenMP
    oracle takes a few seconds per transform."""
    import torch
    O = oracle
    a = _rand(O, 1 << 24, 24)
    d = torch.from_numpy(a.view(np.int64)).cuda()
    for fn in FNS:
        d.copy_(torch.from_numpy(a.view(np.int64)))
        getattr(srs.fft, fn)(d)
        assert np.array_equal(d.cpu().numpy().view(np.uint64), getattr(O, fn)(a)), fn


def test_ntt_asserts(srs):
    with pytest.raises(srs.fft.NotPowerOfTwo):     # src/fft.rs:161
        srs.fft.fft(np.zeros((12, 4), np.uint64))
    with pytest.raises(srs.fft.NotPowerOfTwo):
        srs.fft.ifft(np.zeros((0, 4), np.uint64))


# (max radix bits, k, stride, batch): single workgroup with stride == n and stride > n; two passes; three passes; odd widths; four passes
BATCH_CASES = ((8, 3, 8, 5), (8, 5, 40, 3), (8, 10, 1027, 2), (8, 11, 2056, 3), (4, 12, 4096, 2), (5, 15, (1 << 15) + 8, 2), (4, 16, 1 << 16, 2))
_TRANSFORMS = {"fft": (0, 0), "ifft": (1, 0), "coset_fft": (0, 1), "coset_ifft": (1, 1)}


def _ntt_batch(S, buf, n, stride, batch, fn, device=False):
    """srs_ntt_batch on a copy of `buf` (host words, or the same words in device memory) -> (return code, the buffer afterwards)"""
    from sirius_amd import _lib
    from sirius_amd.commitment import _stream
    inverse, coset = _TRANSFORMS[fn]
    if device:
        import torch
        d = torch.from_numpy(buf.view(np.int64)).cuda()
        rc = _lib.lib().srs_ntt_batch(_lib.FIELD_FR, d.data_ptr(), n, stride, batch, inverse, coset, _lib.SPACE_DEVICE, _stream())
        return rc, d.cpu().numpy().view(np.uint64)
    a = buf.copy()
    rc = _lib.lib().srs_ntt_batch(_lib.FIELD_FR, a.ctypes.data, n, stride, batch, inverse, coset, _lib.SPACE_HOST, _stream())
    return rc, a


def ntt_batch_case(S, O, bits, k, stride, batch, device=False):
    """`batch` vectors of 2^k words, `stride` apart: each becomes the oracle's transform of that vector alone, the words between them stay"""
    from sirius_amd import _lib
    n = 1 << k
    buf = _rand(O, (batch - 1) * stride + n, 500 + k + batch)
    gap = np.ones(buf.shape[0], bool)
    for b in range(batch):
        gap[b * stride:b * stride + n] = False
    assert int(gap.sum()) == (batch - 1) * (stride - n)
    try:
        assert _lib.lib().srs_ntt_set_max_radix_bits(bits) == bits
        for fn in FNS:
            rc, got = _ntt_batch(S, buf, n, stride, batch, fn, device)
            assert rc == _lib.OK, (fn, rc)
            for b in range(batch):
                v = buf[b * stride:b * stride + n]
                assert np.array_equal(got[b * stride:b * stride + n], getattr(O, fn)(v)), (bits, k, stride, batch, fn, b)
            assert np.array_equal(got[gap], buf[gap]), (bits, k, stride, batch, fn)
    finally:
        _lib.lib().srs_ntt_set_max_radix_bits(8)


def ntt_batch_argument_checks(S, O, device=False):
    from sirius_amd import _lib
    buf = _rand(O, 64, 9)
    for n, stride, batch, want in ((16, 15, 2, _lib.ERR_INVALID), (16, 0, 2, _lib.ERR_INVALID), (16, 16, 0, _lib.OK), (16, 3, 0, _lib.OK),
                                   (12, 16, 2, _lib.ERR_NOT_POW2)):
        for fn in ("fft", "coset_ifft"):
            rc, got = _ntt_batch(S, buf, n, stride, batch, fn, device)
            assert rc == want, (n, stride, batch, rc)
            assert np.array_equal(got, buf), (n, stride, batch)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bits,k,stride,batch", BATCH_CASES)
def test_ntt_batch_vs_oracle(srs, oracle, bits, k, stride, batch, device):
    ntt_batch_case(srs, oracle, bits, k, stride, batch, device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ntt_batch_argument_checks(srs, oracle, device):
    ntt_batch_argument_checks(srs, oracle, device)
