"""HyraxPC over ed_on_bls12_381 (JubJub) on one GPU -- the reference's Hyrax381, HyraxPC<EdwardsAffine, DenseMultilinearExtension<Fr>>
(poly-commit/src/hyrax/tests.rs:6,20-21): setup, trim, commit, open and check for ONE polynomial (hyrax/mod.rs:119-168, 176-183,
193-255, 273-406, 418-511), beside te_ipa.py and in the shape of its functions.

Hyrax commits a multilinear polynomial of n variables (n even) as dim = 2^(n/2) Pedersen commitments, one per row of its dim x dim
evaluation matrix.  Here

  setup    dim + 1 generators of b"Hyrax protocol" in one pc_hip_te_sample_generators call; the resident key is com_key || h, which
           already is the extended key of the largest dimension (:143-167; h is the last point, popped at :165)
  commit   all rows in ONE pc_hip_te_msm_many pass over com_key[..dim] || h with scalars row_i || r_i                        (:233-242)
  open     t.row_mul(l) as one pc_hip_te_fr_lincomb over the resident rows (:347), <lt, r> as pc_hip_te_fr_dot (:356), com_d as one
           pc_hip_te_msm over the extended key (:374), z = d + c * lt on the device (:391), the singleton commitments through
           pc_hip_te_point_mul and pc_hip_te_points_sum (:361, :378)
  check    t' = MSM(row_coms, l) over a key made of the row commitments and com(z, z_d) on the device (:501, :504), the two equations
           on the host (:492-493, :505)

The sponge is the caller's (the reference absorbs the key, the row commitments, the point and the three commitments into a generic
CryptographicSponge, :336-342, :381-389), and so is arkworks' serialization of twisted Edwards points: the challenge c is an argument,
and so are the prover's random field elements, in the order the reference draws them -- a test can then replay a restatement of the
scheme bit for bit.  Field elements are 32 Montgomery bytes (uint8), points 64 bytes x || y; the matrix stays in device memory between
commit and open.
"""
import numpy as np

from . import _ffi
from .te_ipa import CURVE, FR_MODULUS, fr_from_int, fr_to_int

PROTOCOL_NAME = b"Hyrax protocol"      # hyrax/mod.rs:26


class InvalidNumberOfVariables(ValueError):
    """hyrax Error::InvalidNumberOfVariables: an odd or missing number of variables, or more than the key supports."""


class IncorrectCommitmentSize(ValueError):
    """hyrax Error::IncorrectCommitmentSize: a commitment whose row count is not 2^(n/2)."""


_RINV = pow(1 << 256, -1, FR_MODULUS)


def _vec_to_int(arr):
    """(k, 32) Montgomery bytes -> list of canonical ints"""
    raw = np.ascontiguousarray(arr, dtype=np.uint8).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") * _RINV % FR_MODULUS for i in range(len(raw) // 32)]


def _vec_to_mont(vals):
    """list of canonical ints -> (k, 32) Montgomery bytes"""
    return np.frombuffer(b"".join((v % FR_MODULUS * (1 << 256) % FR_MODULUS).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def tensor_prime(values):
    """hyrax/utils.rs:27-39 on canonical ints"""
    out = [1]
    for val in reversed(values):
        out = [v * (1 - val) % FR_MODULUS for v in out] + [v * val % FR_MODULUS for v in out]
    return out


def _tensors(point_mont):
    n = len(point_mont)
    point_rev = [fr_to_int(x) for x in reversed(list(point_mont))]                       # :299
    return tensor_prime(point_rev[n // 2:]), tensor_prime(point_rev[:n // 2])            # l, r (:301-307)


def _pedersen_1(g0, h, v_mont, r_mont):
    """the singleton commitment g0 * v + h * r (:361, :378)"""
    return _ffi.te_points_sum(CURVE, np.stack([_ffi.te_point_mul(CURVE, g0, v_mont), _ffi.te_point_mul(CURVE, h, r_mont)]))


class TeHyraxKey:
    """HyraxUniversalParams / CommitterKey / VerifierKey {com_key, h} (hyrax/data_structures.rs) as ONE resident key com_key || h: the
    extended key of dim = len(com_key).  For a polynomial of fewer variables the extended key com_key[..dim] || h is made once per
    dimension and kept."""

    def __init__(self, ctx, full, num_vars):
        self.ctx, self.full, self.num_vars = ctx, full, num_vars
        self.dim = len(full) - 1
        self.g0 = full.read(0, 1)[0].copy()
        self.h = full.read(self.dim, 1)[0].copy()
        self._ext = {}

    def com_key(self):
        """the dim points of com_key on the host (x || y)"""
        return self.full.read(0, self.dim)

    def ext(self, dim):
        if dim == self.dim:
            return self.full
        if dim not in self._ext:
            self._ext[dim] = self.ctx.upload_te_srs(CURVE, np.concatenate([self.full.read(0, dim), self.h[None]]))
        return self._ext[dim]

    def close(self):
        for s in self._ext.values():
            s.free()
        self._ext = {}
        if self.full is not None:
            self.full.free()
            self.full = None


def setup(ctx, num_vars):
    """HyraxPC::setup (hyrax/mod.rs:119-168): 2^(num_vars / 2) + 1 generators of PROTOCOL_NAME from index 0, sampled on the device;
    the last one is h."""
    if num_vars is None or num_vars < 0 or num_vars % 2 == 1:                             # :124-134
        raise InvalidNumberOfVariables(f"{num_vars} variables")
    dim = 1 << (num_vars // 2)
    return TeHyraxKey(ctx, ctx.te_sample_generators(CURVE, PROTOCOL_NAME, 0, dim + 1), num_vars)


def trim(pp):
    """HyraxPC::trim (hyrax/mod.rs:176-183): a clone -- the committer and the verifier key are the parameters themselves"""
    return pp, pp


def commit(key, evals_dev, rands_mont):
    """HyraxPC::commit for one polynomial (hyrax/mod.rs:213-252).  evals_dev: torch cuda uint8 (2^n, 32), the polynomial's evaluations
    (DenseMultilinearExtension::to_evaluations), Montgomery; rands_mont: (dim, 32) the row randomisers (the reference draws them inside
    the row loop).  Returns (row_coms (dim, 64) uint8, state) with state = (rands, the matrix rows on the device)."""
    import torch
    total = evals_dev.shape[0]
    n = total.bit_length() - 1
    if total != 1 << n or n % 2 == 1 or n > key.dim:                                     # :220-228 (the reference compares n with com_key.len())
        raise InvalidNumberOfVariables(f"{n} variables")
    dim = 1 << (n // 2)
    if dim > key.dim:
        raise InvalidNumberOfVariables(f"{n} variables need {dim} generators, the key has {key.dim}")
    rands_mont = np.ascontiguousarray(rands_mont, dtype=np.uint8).reshape(dim, 32)
    # flat_to_matrix_column_major (hyrax/utils.rs:13-21): row r = flat[r], flat[dim + r], ...
    mat = evals_dev.view(dim, dim, 32).transpose(0, 1).contiguous()
    rd = torch.from_numpy(rands_mont).to(evals_dev.device)
    ext = torch.cat([mat, rd.view(dim, 1, 32)], dim=1).contiguous()                       # row_i || r_i
    row_coms, _ = key.ext(dim).msm_many(ext, m=dim + 1, n_msms=dim, montgomery=True)      # :233-242
    return row_coms, (rands_mont, mat)


def open(key, state, point_mont, r_eval, d_mont, r_d, r_b, c):   # noqa: A001 (the reference's name)
    """HyraxPC::open for one polynomial (hyrax/mod.rs:287-402).  r_eval, d_mont (dim, 32), r_d, r_b: the random elements in the order
    the reference draws them (:360, :367-368, :373, :377); c: the sponge's challenge (:389).  Returns the HyraxProof fields (com_eval,
    com_d, com_b, z (dim, 32), z_d, z_b) and the evaluation, all Montgomery bytes."""
    import torch
    ctx = key.ctx
    rands, mat = state
    dim = mat.shape[0]
    n = len(point_mont)
    if n % 2 == 1 or 1 << (n // 2) != dim:
        raise InvalidNumberOfVariables(f"point of {n} variables, matrix of dimension {dim}")
    l, r = _tensors(point_mont)
    dev = mat.device
    lt = torch.empty((dim, 32), dtype=torch.uint8, device=dev)
    ctx.te_fr_lincomb(CURVE, [mat.data_ptr() + 32 * dim * i for i in range(dim)], _vec_to_mont(l), n_out=dim, out=lt, lens=[dim] * dim)      # :347
    r_lt = sum(a * b for a, b in zip(l, _vec_to_int(rands))) % FR_MODULUS                 # :351-354
    r_dev = torch.from_numpy(_vec_to_mont(r)).to(dev)
    ev = ctx.te_fr_dot(CURVE, lt, r_dev, dim)                                            # :356
    com_eval = _pedersen_1(key.g0, key.h, ev, np.ascontiguousarray(r_eval, dtype=np.uint8))                                              # :361
    d_mont = np.ascontiguousarray(d_mont, dtype=np.uint8).reshape(dim, 32)
    b = sum(a * x for a, x in zip(r, _vec_to_int(d_mont))) % FR_MODULUS                   # :370
    d_ext = torch.from_numpy(np.concatenate([d_mont, np.asarray(r_d, dtype=np.uint8).reshape(1, 32)])).to(dev)
    com_d = key.ext(dim).msm(d_ext, n=dim + 1, montgomery=True)[0]                       # :374
    com_b = _pedersen_1(key.g0, key.h, fr_from_int(b), np.ascontiguousarray(r_b, dtype=np.uint8))                                        # :378
    z = torch.empty((dim, 32), dtype=torch.uint8, device=dev)
    ctx.te_fr_lincomb(CURVE, [d_ext, lt], np.stack([fr_from_int(1), np.asarray(c, dtype=np.uint8)]), n_out=dim, out=z, lens=[dim, dim])   # :391
    ci = fr_to_int(c)
    z_d = fr_from_int(ci * r_lt + fr_to_int(r_d))                                        # :392
    z_b = fr_from_int(ci * fr_to_int(r_eval) + fr_to_int(r_b))                           # :393
    return (com_eval, com_d, com_b, z.cpu().numpy(), z_d, z_b), ev


def check(key, row_coms, point_mont, proof, c):
    """HyraxPC::check for one commitment (hyrax/mod.rs:430-511): equation (14) on the host (:492-495), then t' = MSM(row_coms, l) and
    the commitment of (z, z_d) on the device for equation (13) (:501-507).  Returns bool."""
    import torch
    ctx = key.ctx
    n = len(point_mont)
    if n % 2 == 1:
        raise InvalidNumberOfVariables(f"{n} variables")
    dim = 1 << (n // 2)
    row_coms = np.ascontiguousarray(row_coms, dtype=np.uint8)
    if row_coms.shape[0] != dim:                                                         # :463-468
        raise IncorrectCommitmentSize(f"encountered {row_coms.shape[0]}, expected {dim}")
    com_eval, com_d, com_b, z, z_d, z_b = proof
    l, r = _tensors(point_mont)
    c = np.ascontiguousarray(c, dtype=np.uint8)
    z = np.ascontiguousarray(z, dtype=np.uint8).reshape(dim, 32)
    ip = sum(a * x for a, x in zip(r, _vec_to_int(z))) % FR_MODULUS
    com_dp = _pedersen_1(key.g0, key.h, fr_from_int(ip), np.ascontiguousarray(z_b, dtype=np.uint8))                                      # :492
    if not (com_dp == _ffi.te_points_sum(CURVE, np.stack([_ffi.te_point_mul(CURVE, np.ascontiguousarray(com_eval, dtype=np.uint8), c),
                                                           np.ascontiguousarray(com_b, dtype=np.uint8)]))).all():
        return False
    rows = ctx.upload_te_srs(CURVE, row_coms)
    try:
        l_dev = torch.from_numpy(_vec_to_mont(l)).cuda()
        t_prime = rows.msm(l_dev, n=dim, montgomery=True)[0]                             # :501
    finally:
        rows.free()
    z_ext = torch.from_numpy(np.concatenate([z, np.asarray(z_d, dtype=np.uint8).reshape(1, 32)])).cuda()
    com_z_zd = key.ext(dim).msm(z_ext, n=dim + 1, montgomery=True)[0]                    # :504
    return bool((com_z_zd == _ffi.te_points_sum(CURVE, np.stack([_ffi.te_point_mul(CURVE, t_prime, c), np.ascontiguousarray(com_d, dtype=np.uint8)]))).all())
