"""InnerProductArgPC::setup / trim over ed_on_bls12_381 without a device: the Python restatement of sample_generators
(tests/harness/te_setup.py) against the figures recorded when it was first written, from_random_bytes on crafted inputs, the kernel
bodies of csrc/te_setup.hpp through the host build of the probe (tests/hip/probe_te_setup.hip; the case tables of
tests/harness/tesetupprobe.py, which tests/test_te_setup_gpu.py runs on the device), and the arithmetic of setup and trim."""
import pytest

from harness import te_setup as S
from harness import teref as E
from harness import tesetupprobe as P

Q = E.Q
NAME = S.PROTOCOL_NAME


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def test_generators_lie_in_the_prime_order_subgroup():
    for i in list(range(256)) + list(range(1000, 1016)):
        g, _ = S.generator(NAME, i)
        assert E.on_curve(g) and g != E.IDENT and E.mul(E.R, g) == E.IDENT, i


def test_digest_outcomes_of_the_first_indices():
    want = {0: [S.ACCEPT], 1: [S.ACCEPT], 3: [S.RANGE, S.ACCEPT], 4: [S.RANGE, S.NON_SQUARE, S.NON_SQUARE, S.ACCEPT], 6: [S.NON_SQUARE, S.ACCEPT]}
    for i, reasons in want.items():
        g, h, got = S.trace(NAME, i)
        assert got == reasons and S.generator(NAME, i)[1] == len(reasons), i
    assert S.trace(NAME, 0)[1][31] >> 7 == 1 and S.trace(NAME, 1)[1][31] >> 7 == 0          # flag set, flag clear
    assert S.generator(NAME, 1008)[1] == 16
    # the retry with j = 0 is another message than the first digest
    assert S.digest(NAME, 3) != S.digest(NAME, 3, 0) and S.try_bytes(S.digest(NAME, 3, 0))[1] == S.ACCEPT


def test_leading_digits_of_generators_0_and_4():
    g0, g4 = S.generator(NAME, 0)[0], S.generator(NAME, 4)[0]
    assert ("%064x" % g0[0]).startswith("47da5cfd7a53e08d") and ("%064x" % g0[1]).startswith("253026c35d6a9cd0")
    assert ("%064x" % g4[0]).startswith("401658b199919be7") and ("%064x" % g4[1]).startswith("162aa860317039ad")


def test_accepted_digest_gives_y_and_the_sign_of_x():
    for i in range(64):
        (x, y), h, _ = S.trace(NAME, i)
        v = int.from_bytes(h, "little")
        assert y == v & ((1 << 255) - 1) and (x > Q - x) == bool(v >> 255), i
        assert E.on_curve((x, y))


# ---- from_random_bytes on crafted inputs ---------------------------------------------------------------------------------------------

def test_from_random_bytes_crafted():
    for flag in (0, 1):
        p, why = S.try_bytes(P.crafted(Q - 1, flag))                 # x^2 = 0: the point of order 2 either way
        assert why == S.ACCEPT and p == (0, Q - 1) == E.T2 and E.mul(8, p) == E.IDENT
        p, why = S.try_bytes(P.crafted(1, flag))                     # x^2 = 0 again: the identity
        assert why == S.ACCEPT and p == E.IDENT
        assert S.try_bytes(P.crafted(Q, flag)) == (None, S.RANGE)
        assert S.try_bytes(P.crafted((1 << 255) - 1, flag)) == (None, S.RANGE)
        assert S.try_bytes(P.crafted(P.y_with(False), flag)) == (None, S.NON_SQUARE)
    lo, hi = S.try_bytes(P.crafted(0, 0))[0], S.try_bytes(P.crafted(0, 1))[0]      # y = 0: the two points of order 4
    assert {lo, hi} == {E.T4, E.neg(E.T4)} and lo[0] < hi[0] and E.mul(2, lo) == E.T2 == E.mul(2, hi)
    y = P.y_with(True)
    lo, hi = S.try_bytes(P.crafted(y, 0))[0], S.try_bytes(P.crafted(y, 1))[0]
    assert lo[1] == hi[1] == y and lo[0] + hi[0] == Q and lo[0] < hi[0] and E.on_curve(lo) and E.on_curve(hi)


# ---- the kernel bodies through the host build ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    return P.T.host_probe()


def test_probe_sqrt(host):
    assert P.check_sqrt(host, host) == 4 + 33 * 3


def test_probe_digest(host):
    assert P.check_digest(host, host) == 3 * (5 + 5 * 3)


def test_probe_from_random_bytes(host):
    assert P.check_try(host, host) == 14 + sum(S.generator(NAME, i)[1] for i in range(16))


def test_probe_sample_body(host):
    assert P.check_sample(host, host) == 64 + 1 + 2


# ---- setup / trim --------------------------------------------------------------------------------------------------------------------

def test_setup_and_trim_arithmetic():
    assert [S.pow2_at_least(n) for n in (0, 1, 2, 3, 4, 5, 201, 256, 257)] == [1, 1, 2, 4, 4, 8, 256, 256, 512]
    pp = S.setup(5)                                                   # 5 + 1 -> 8 coefficients: generators 0..7, s = 8, h = 9
    assert pp["max_degree"] == 7 and len(pp["comm_key"]) == 8
    assert pp["comm_key"] == [S.generator(NAME, i)[0] for i in range(8)]
    assert pp["s"] == S.generator(NAME, 8)[0] and pp["h"] == S.generator(NAME, 9)[0]
    assert S.setup(7)["h"] == pp["h"] and S.setup(0)["h"] == S.generator(NAME, 2)[0]
    ck = S.trim(pp, 2)                                                # 2 + 1 -> 4
    assert ck["supported_degree"] == 3 and ck["comm_key"] == pp["comm_key"][:4] and (ck["s"], ck["h"]) == (pp["s"], pp["h"])
    assert len(S.trim(pp, 7)["comm_key"]) == 8 and len(S.trim(pp, 4)["comm_key"]) == 8
    with pytest.raises(ValueError, match="TrimmingDegreeTooLarge"):
        S.trim(pp, 8)
