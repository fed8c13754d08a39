"""InnerProductArgPC over ed_on_bls12_381 (JubJub) on one GPU: open and check for ONE polynomial, without hiding and without a degree
bound (poly-commit/src/ipa_pc/mod.rs:475-723, 725-773), in the shape of ipa.py's ipa_open / ipa_check.  The committer key is a
resident TeSrs and is never modified; the halving rounds run inside the library (pc_hip_te_ipa_open_rounds), the Blake2s transcript
(`compute_random_oracle_challenge`, :74-87, :615-625, :681-688) is host work on two points per round and lives here.

Byte conventions of the transcript: those of ark-serialize / ark-ff / ark-ec 0.5, restated from the crates' published behaviour next
to the ones in host/transcript.hpp and, like them, NOT yet confirmed against the crates:
  field element      canonical residue, little-endian, 32 bytes (both the 255-bit coordinate field and the 252-bit scalar field)
  TE affine point    serialize_uncompressed: x, then y, each a canonical little-endian residue in 32 bytes; no flag bits (the flags of
                     twisted_edwards::Affine belong to the compressed form only)
  from_random_bytes  the 32 bytes little-endian with the top 4 bits cleared (252-bit modulus); None at >= r

setup and trim (ipa_pc/mod.rs:344-400) make the key on the device: sample_generators is one call of the library
(pc_hip_te_sample_generators), whose from_random_bytes for twisted_edwards::Affine is restated in csrc/te_setup.hpp and, like the
conventions above, NOT confirmed against the crates.
"""
import hashlib

import numpy as np

from . import _ffi

CURVE = "ed_on_bls12_381"
FQ_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # the coordinate field: BLS12-381's Fr
FR_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7      # the prime subgroup order, 252 bits
_R = 1 << 256


def fr_to_int(mont_bytes):
    return int.from_bytes(np.asarray(mont_bytes, dtype=np.uint8).tobytes(), "little") * pow(_R, -1, FR_MODULUS) % FR_MODULUS


def fr_from_int(v):
    return np.frombuffer((v % FR_MODULUS * _R % FR_MODULUS).to_bytes(32, "little"), dtype=np.uint8).copy()


def ser_fr(mont_bytes):
    return fr_to_int(mont_bytes).to_bytes(32, "little")


def ser_point(xy_mont):
    b = np.asarray(xy_mont, dtype=np.uint8).tobytes()
    ri = pow(_R, -1, FQ_MODULUS)
    x, y = int.from_bytes(b[:32], "little") * ri % FQ_MODULUS, int.from_bytes(b[32:64], "little") * ri % FQ_MODULUS
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def from_random_bytes(digest):
    """Field::from_random_bytes for the 252-bit scalar field: the integer, or None at >= r"""
    v = int.from_bytes(digest[:32], "little") & ((1 << 252) - 1)
    return v if v < FR_MODULUS else None


def random_oracle_challenge(data):
    """compute_random_oracle_challenge with D = Blake2s: the challenge as 32 Montgomery bytes"""
    i = 0
    while True:
        v = from_random_bytes(hashlib.blake2s(data + i.to_bytes(8, "little")).digest())
        if v is not None:
            return fr_from_int(v)
        i += 1


PROTOCOL_NAME = b"PC-DL-2020"


def _pow2_at_least(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def setup(ctx, max_degree, protocol_name=PROTOCOL_NAME):
    """InnerProductArgPC::setup (ipa_pc/mod.rs:344-366): max_degree + 1 is rounded up to a power of two and max_degree + 3 generators
    are sampled on the device.  Returns the UniversalParams as a dict: comm_key, a resident TeSrs of max_degree + 1 points; s and h,
    generators max_degree + 1 and max_degree + 2 (the reference pops h first: it is the last one) as 64 host bytes x || y; max_degree."""
    max_degree = _pow2_at_least(max_degree + 1) - 1
    gens = ctx.te_sample_generators(CURVE, protocol_name, 0, max_degree + 3)
    try:
        tail = gens.read(max_degree + 1, 2)
        comm_key = gens.prefix(max_degree + 1)
    finally:
        gens.free()
    return dict(comm_key=comm_key, s=tail[0].copy(), h=tail[1].copy(), max_degree=max_degree)


def trim(pp, supported_degree):
    """InnerProductArgPC::trim (ipa_pc/mod.rs:368-400): supported_degree + 1 is rounded up to a power of two; the committer key is the
    prefix of pp's (a resident key of its own, pp is untouched).  The committer and the verifier key hold the same values: one dict."""
    supported_degree = _pow2_at_least(supported_degree + 1) - 1
    if supported_degree > pp["max_degree"]:
        raise ValueError("TrimmingDegreeTooLarge")
    return dict(comm_key=pp["comm_key"].prefix(supported_degree + 1), s=pp["s"], h=pp["h"], supported_degree=supported_degree,
                max_degree=pp["max_degree"])


def ipa_open(ctx, comm_key, h_xy, coeffs_dev, comm, point_mont, opening_challenge, fixed_key_below=0, timings=None):
    """InnerProductArgPC::open for one polynomial of n = len(comm_key) coefficients (a power of two).  comm_key: a resident TeSrs;
    coeffs_dev: torch cuda uint8 tensor (n, 32), Montgomery, left as it is; comm: the polynomial's commitment (64 bytes); point_mont,
    opening_challenge: 32 Montgomery bytes.  Returns ((l_vec, r_vec, final_comm_key, c), first round challenge)."""
    import torch
    n = len(comm_key)
    assert n and n & (n - 1) == 0 and tuple(coeffs_dev.shape) == (n, 32)
    xi = np.ascontiguousarray(opening_challenge, dtype=np.uint8)
    # the combined polynomial xi * p and its value at the point with the round kernels alone: over c2 = (0 | p) and z2 = (powers | 0)
    # the "left" inner product at size 2n is <p, powers> = p(z), and a fold at size 2n by u^-1 = xi leaves xi * p in the lower half
    c2 = torch.cat([torch.zeros_like(coeffs_dev), coeffs_dev]).contiguous()
    z2 = torch.zeros_like(c2)
    ctx.te_fr_powers(CURVE, point_mont, n, z2)
    v = fr_from_int(fr_to_int(ctx.te_ipa_fold_dots(CURVE, c2, z2, 2 * n)[0]) * fr_to_int(xi))
    ctx.te_ipa_fold_dots(CURVE, c2, z2, n, u=xi, u_inv=xi)
    ccomm = _ffi.te_point_mul(CURVE, np.ascontiguousarray(comm, dtype=np.uint8), xi)
    rc = random_oracle_challenge(ser_point(ccomm) + ser_fr(point_mont) + ser_fr(v))
    h_prime = _ffi.te_point_mul(CURVE, np.ascontiguousarray(h_xy, dtype=np.uint8), rc)
    state = {"rc": rc}

    def next_challenge(l, r):
        state["rc"] = random_oracle_challenge(ser_fr(state["rc"]) + ser_point(l) + ser_point(r))
        return state["rc"]
    out = comm_key.ipa_open_rounds(c2, n, point_mont, h_prime, next_challenge, fixed_key_below, want_times=timings is not None)
    if timings is not None:
        timings["per_round_ms"], timings["ec_fold_per_round_ms"] = [round(x, 3) for x in out[4]], [round(x, 3) for x in out[5]]
    return tuple(out[:4]), rc


def succinct_check_eval(challenges_mont, point_mont):
    """SuccinctCheckPolynomial::evaluate (ipa_pc/data_structures.rs:223-236): prod_i (1 + u_i z^(2^(log_d - i))), the integer"""
    z, log_d, prod = fr_to_int(point_mont), len(challenges_mont), 1
    for i, u in enumerate(challenges_mont, start=1):
        prod = prod * (1 + pow(z, 1 << (log_d - i), FR_MODULUS) * fr_to_int(u)) % FR_MODULUS
    return prod


def ipa_check(ctx, comm_key, h_xy, comm, point_mont, value_mont, proof, opening_challenge):
    """InnerProductArgPC::check for one commitment: the succinct check on the host and the MSM of the committer key with the check
    polynomial's coefficients on the device, the coefficients made there as the per-base factors the key folds would apply
    (pc_hip_te_ipa_key_scalars folding ones by every challenge).  proof = (l_vec, r_vec, final_comm_key, c).  Returns bool."""
    import torch
    l_vec, r_vec, final_key, c = proof
    n = len(comm_key)
    log_d = (n - 1).bit_length()
    if len(l_vec) != len(r_vec) or len(l_vec) != log_d:
        raise ValueError(f"IncorrectInputLength: expected proof vectors to be {log_d}, l_vec {len(l_vec)}, r_vec {len(r_vec)}")
    pm = lambda p, k: _ffi.te_point_mul(CURVE, np.ascontiguousarray(p, dtype=np.uint8), np.ascontiguousarray(k, dtype=np.uint8))      # noqa: E731
    xi = np.ascontiguousarray(opening_challenge, dtype=np.uint8)
    combined_v = fr_from_int(fr_to_int(xi) * fr_to_int(value_mont))
    ccomm = pm(comm, xi)
    rc = random_oracle_challenge(ser_point(ccomm) + ser_fr(point_mont) + ser_fr(combined_v))
    h_prime = pm(h_xy, rc)
    terms = [ccomm, pm(h_prime, combined_v)]
    chal = []
    for l, r in zip(l_vec, r_vec):
        rc = random_oracle_challenge(ser_fr(rc) + ser_point(l) + ser_point(r))
        chal.append(rc)
        terms.append(pm(l, fr_from_int(pow(fr_to_int(rc), -1, FR_MODULUS))))
        terms.append(pm(r, rc))
    round_comm = _ffi.te_points_sum(CURVE, np.stack(terms))
    v_prime = fr_from_int(succinct_check_eval(chal, point_mont) * fr_to_int(c))
    check_elem = _ffi.te_points_sum(CURVE, np.stack([pm(final_key, c), pm(h_prime, v_prime)]))
    if not (round_comm == check_elem).all():
        return False
    s_dev = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    ctx.te_fr_powers(CURVE, fr_from_int(1), n, s_dev)
    m = n
    for u in chal:                                           # coefficient j picks up u_i iff bit (log_d - i) of j is set
        ctx.te_ipa_key_scalars(CURVE, None, 0, s_dev, n, fold_u=u, fold_m=m)
        m //= 2
    key = comm_key.msm(s_dev, n=n, base_offset=0, montgomery=True)[0]
    return bool((key == np.asarray(final_key)).all())
