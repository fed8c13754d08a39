"""setup and trim of InnerProductArgPC (poly-commit/src/ipa_pc/mod.rs:344-400) and setup of HyraxPC (hyrax/mod.rs:119-168) over the
short Weierstrass curves of the library (bls12_381, bn254, pallas, bls12_377) on one GPU: the keys that ipa.py's ipa_open / ipa_check and a
Hyrax commit / open / check run against, made on the device instead of from known scalars.

sample_generators is one call of the library (pc_hip_sample_generators: Blake2s256, from_random_bytes with its square root, the
cofactor, normalize_batch).  short_weierstrass::Affine::from_random_bytes -- where the two flag bits of a base field sit, and which of
the two roots a flag names -- is restated in csrc/sw_setup.hpp from the published behaviour of ark-ec / ark-ff 0.5 and, like the
conventions of te_ipa.py, NOT confirmed against the crates.  Either root gives a valid key; only bit parity with a key arkworks made
rests on it.
"""
IPA_PROTOCOL_NAME = b"PC-DL-2020"          # InnerProductArgPC::PROTOCOL_NAME
HYRAX_PROTOCOL_NAME = b"Hyrax protocol"    # hyrax/mod.rs PROTOCOL_NAME


def _pow2_at_least(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def ipa_setup(ctx, curve, max_degree, protocol_name=IPA_PROTOCOL_NAME):
    """InnerProductArgPC::setup (ipa_pc/mod.rs:344-366): max_degree + 1 is rounded up to a power of two and max_degree + 3 generators
    are sampled on the device.  Returns the UniversalParams as a dict: comm_key, a resident Srs of max_degree + 1 points; s and h,
    generators max_degree + 1 and max_degree + 2 (the reference pops h first: it is the last one) as host arrays x || y of uint64
    Montgomery limbs; max_degree; curve."""
    max_degree = _pow2_at_least(max_degree + 1) - 1
    gens = ctx.sample_generators(curve, protocol_name, 0, max_degree + 3)
    try:
        tail = gens.read(max_degree + 1, 2)
        comm_key = gens.prefix(max_degree + 1)
    finally:
        gens.free()
    return dict(comm_key=comm_key, s=tail[0].copy(), h=tail[1].copy(), max_degree=max_degree, curve=curve)


def ipa_trim(pp, supported_degree):
    """InnerProductArgPC::trim (ipa_pc/mod.rs:368-400): supported_degree + 1 is rounded up to a power of two; the committer key is the
    prefix of pp's (a resident key of its own, pp is untouched).  The committer and the verifier key hold the same values: one dict."""
    supported_degree = _pow2_at_least(supported_degree + 1) - 1
    if supported_degree > pp["max_degree"]:
        raise ValueError("TrimmingDegreeTooLarge")
    return dict(comm_key=pp["comm_key"].prefix(supported_degree + 1), s=pp["s"], h=pp["h"], supported_degree=supported_degree,
                max_degree=pp["max_degree"], curve=pp["curve"])


def hyrax_setup(ctx, curve, num_vars):
    """HyraxPC::setup (hyrax/mod.rs:119-168): dim + 1 points with dim = 2^(num_vars / 2) under b"Hyrax protocol", the last one is h.
    A missing or odd num_vars raises ValueError("InvalidNumberOfVariables"), where the reference returns that error.  Returns the
    HyraxUniversalParams as a dict of host arrays of uint64 Montgomery limbs: com_key (dim, x || y) and h (x || y)."""
    if num_vars is None or num_vars % 2 == 1:
        raise ValueError("InvalidNumberOfVariables")
    dim = 1 << (num_vars // 2)
    gens = ctx.sample_generators(curve, HYRAX_PROTOCOL_NAME, 0, dim + 1)
    try:
        pts = gens.read(0, dim + 1)
    finally:
        gens.free()
    return dict(com_key=pts[:dim].copy(), h=pts[dim].copy(), num_vars=num_vars, curve=curve)
