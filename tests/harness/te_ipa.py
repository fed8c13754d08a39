"""Pure-Python restatement of InnerProductArgPC over ed_on_bls12_381 for the tests of the device path (abi_te_ipa.hip, te_ipa.py): the
Fr vector steps of the halving rounds, the Blake2s transcript, the whole `open` for one polynomial without hiding or degree bound
(ipa_pc/mod.rs:475-723), `succinct_check` / `check` (:91-203, :725-773), the fold table and the subgroup check -- over harness/teref.py,
on Python integers.  Scalars are integers in [0, r); a point is teref's (x, y).  Group products are integer-exact (teref.mul / msm
never use r P = O), so keys with points outside the prime-order subgroup have well-defined expected values, the ones the FOLDING
route of the device computes."""
import hashlib

import numpy as np

from . import teref as E

R = E.R
FOLD_ROWS = 253


# ---- Fr vectors ----------------------------------------------------------------------------------------------------------------
def powers(z, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * z % R
    return out


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def fold_dots(c, z, m, u=None, ui=None):
    """pc_hip_te_ipa_fold_dots on lists: the optional fold at size 2m in place, then (<c[m/2..m), z[0..m/2)>, <c[0..m/2), z[m/2..m)>)"""
    if u is not None:
        for t in range(m):
            c[t] = (c[t] + ui * c[t + m]) % R
            z[t] = (z[t] + u * z[t + m]) % R
    h = m // 2
    return (dot(c[h:m], z[:h]), dot(c[:h], z[h:m])) if h else (0, 0)


def key_scalars_fold(s, fold_m, u):
    """IpaKeyScalarUpdateBody: s_j *= u where (j mod fold_m) >= fold_m / 2"""
    return [v * u % R if (j & (fold_m - 1)) >= fold_m // 2 else v for j, v in enumerate(s)]


def key_scalars_lr(c, s, m):
    """IpaFixedKeyScalarsBody: the scalar vectors of L and R over the fixed key for the round at size m"""
    h, out_l, out_r = m // 2, [], []
    for j, sj in enumerate(s):
        i = j & (m - 1)
        v = c[h + i if i < h else i - h] * sj % R
        out_l.append(v if i < h else 0)
        out_r.append(0 if i < h else v)
    return out_l, out_r


def fr_bytes(v):
    """32 Montgomery bytes of the integer v"""
    return np.frombuffer((v % R * E.MONT_R % R).to_bytes(32, "little"), dtype=np.uint8).copy()


def fr_int(b):
    return int.from_bytes(np.asarray(b, dtype=np.uint8).tobytes(), "little") * pow(E.MONT_R, -1, R) % R


# ---- transcript (ipa_pc/mod.rs:74-87, 615-625, 681-688) ---------------------------------------------------------------------------
def ser_fr(v):
    return v.to_bytes(32, "little")


def ser_point(p):
    x, y = E.IDENT if p == E.ZERO else p
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def from_random_bytes(digest):
    v = int.from_bytes(digest[:32], "little") & ((1 << 252) - 1)
    return v if v < R else None


def challenge(data):
    i = 0
    while True:
        v = from_random_bytes(hashlib.blake2s(data + i.to_bytes(8, "little")).digest())
        if v is not None:
            return v
        i += 1


# ---- open / check ----------------------------------------------------------------------------------------------------------------
def open_rounds(key, coeffs, z, h_prime, rc):
    """the halving loop, ipa_pc/mod.rs:664-711, folding the key in every round: (l_vec, r_vec, final_comm_key, c)"""
    n = len(coeffs)
    c, zs, key = list(coeffs), powers(z, n), list(key[:n])
    l_vec, r_vec = [], []
    while n > 1:
        h = n // 2
        l = E.add(E.msm(key[:h], c[h:n]), E.mul(dot(c[h:n], zs[:h]), h_prime))
        r = E.add(E.msm(key[h:n], c[:h]), E.mul(dot(c[:h], zs[h:n]), h_prime))
        l_vec.append(l)
        r_vec.append(r)
        rc = challenge(ser_fr(rc) + ser_point(l) + ser_point(r))
        ui = pow(rc, -1, R)
        c = [(c[i] + ui * c[h + i]) % R for i in range(h)]
        zs = [(zs[i] + rc * zs[h + i]) % R for i in range(h)]
        key = E.fold(key[:n], rc)
        n = h
    kf = key[0]
    return l_vec, r_vec, (E.IDENT if kf == E.ZERO else kf), c[0]


def open(key, h, coeffs, comm, z, xi):
    """InnerProductArgPC::open for one polynomial: ((l_vec, r_vec, final_comm_key, c), first round challenge)"""
    comb = [xi * v % R for v in coeffs]
    ccomm = E.mul(xi, comm)
    v = dot(comb, powers(z, len(comb)))
    rc = challenge(ser_point(ccomm) + ser_fr(z) + ser_fr(v))
    return open_rounds(key, comb, z, E.mul(rc, h), rc), rc


def check(key, h, comm, z, value, proof, xi):
    """InnerProductArgPC::check for one commitment (succinct_check and the final key), with the key's points in the prime-order subgroup"""
    l_vec, r_vec, final_key, c = proof
    n = len(key)
    log_d = (n - 1).bit_length()
    if len(l_vec) != log_d or len(r_vec) != log_d:
        return False
    combined_v = xi * value % R
    ccomm = E.mul(xi, comm)
    rc = challenge(ser_point(ccomm) + ser_fr(z) + ser_fr(combined_v))
    h_prime = E.mul(rc, h)
    round_comm = E.add(ccomm, E.mul(combined_v, h_prime))
    chal = []
    for l, r in zip(l_vec, r_vec):
        rc = challenge(ser_fr(rc) + ser_point(l) + ser_point(r))
        chal.append(rc)
        round_comm = E.add(round_comm, E.add(E.mul(pow(rc, -1, R), l), E.mul(rc, r)))
    ev = 1
    for i, u in enumerate(chal, start=1):
        ev = ev * (1 + pow(z, 1 << (log_d - i), R) * u) % R
    if round_comm != E.add(E.mul(c, final_key), E.mul(ev * c % R, h_prime)):
        return False
    s = [1] * n
    m = n
    for u in chal:
        s = key_scalars_fold(s, m, u)
        m //= 2
    return E.msm(key, s) == final_key


# ---- the fold table and the subgroup check -----------------------------------------------------------------------------------------
def fold_table(key, rows=FOLD_ROWS):
    """T[b][j] = 2^b * key[n/2 + j]; an all-zero entry stays in row 0 and is the identity from row 1 on"""
    half = len(key) // 2
    row = list(key[half:])
    out = [row]
    for _ in range(rows - 1):
        row = [E.mul(2, p) for p in row]
        out.append(row)
    return out


def in_subgroup(key):
    return all(E.mul(R, p) == E.IDENT for p in key)
