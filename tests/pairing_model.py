"""Pure-Python model of the optimal-ate pairing check of bls_kernels.hip -- TEST INFRASTRUCTURE ONLY.

Values are those of oracle/g1.py and oracle/g2.py (ints, Fp2 tuples, None = infinity).

Tower.  Fp2 = Fp[u]/(u^2 + 1), xi = 1 + u, Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v).  Since v = w^2 the same field is
Fp2[w]/(w^6 - xi), and an Fp12 value is held FLAT: a list of six Fp2 coefficients c_0 .. c_5 of w^0 .. w^5; c_(2i+j) is the
coefficient of v^i w^j of the tower.  The kernel gives coefficient k to lane pair k of a 16-lane row.

What the kernel executes is not restated here by hand a second time: the point steps of the Miller loop (DBL_PROG, ADD_PROG)
and the whole final exponentiation (final_exp_program()) are small op tables; tests/golden/generate_pairing.py writes them into
pos_evolution_amd/csrc/bls_consts.inc, the kernels interpret them, and this model interprets the same tables.

Final power: the result is e(P, Q)^c with c = 3, i.e. f^((p^12 - 1) / r * 3): the hard part uses
3 (p^4 - p^2 + 1) / r = (z - 1)^2 (z + p) (z^2 + p^2 - 1) + 3; gcd(3, r) = 1, so "== 1" is unchanged.
"""
from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from oracle.g2 import F2_ONE, F2_ZERO, f2_add, f2_mul, f2_neg, f2_sqr, f2_sub, f2_inv

XI = (1, 1)
Z_ABS = 0xD201000000010000          # |z|; z is negative
FINAL_POWER_C = 3


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_mul_xi(a):
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2_pow(a, e):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


# ---- Fp12, flat over w ---------------------------------------------------------------------------------------------
F12_ONE = [F2_ONE] + [F2_ZERO] * 5


def f12_mul(a, b):
    out = []
    for k in range(6):
        s, w = F2_ZERO, F2_ZERO                      # products below w^6 | products that wrap (times xi)
        for i in range(6):
            t = f2_mul(a[i], b[(k - i) % 6])
            if i <= k:
                s = f2_add(s, t)
            else:
                w = f2_add(w, t)
        out.append(f2_add(s, f2_mul_xi(w)))
    return out


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    """a^(p^6): w -> -w."""
    return [f2_neg(c) if k & 1 else c for k, c in enumerate(a)]


def frobenius_constants():
    """FROB[n - 1][k] = xi^(k (p^n - 1) / 6), n = 1, 2, 3: (sum c_k w^k)^(p^n) = sum c_k^(p^n) FROB[n-1][k] w^k.
    Derived from p and the tower alone."""
    return [[f2_pow(XI, k * (P ** n - 1) // 6) for k in range(6)] for n in (1, 2, 3)]


FROB = frobenius_constants()


def f12_frob(a, n):
    return [f2_mul(f2_conj(c) if n & 1 else c, FROB[n - 1][k]) for k, c in enumerate(a)]


# which coefficient pair (x, y) = (c_j, c_(j+3)) lane pair k squares as an Fp4 value x + y s (s = w^3, s^2 = xi), and what
# it keeps of (x + y s)^2 = lo + hi s:   0: lo   1: hi   2: xi * hi
CYCLO_J = (0, 2, 1, 0, 2, 1)
CYCLO_PART = (0, 2, 0, 1, 0, 1)
CYCLO_SIGN = (-1, 1, -1, 1, -1, 1)   # out_k = 3 part + sign * 2 c_k


def f12_cyclo_sqr(a):
    """Granger-Scott squaring, valid in the cyclotomic subgroup (after the easy part): with A_i = c_i + c_(i+3) s,
    a^2 = (3 A_0^2 - 2 conj A_0) + (3 s A_2^2 + 2 conj A_1) w + (3 A_1^2 - 2 conj A_2) w^2."""
    out = []
    for k in range(6):
        x, y = a[CYCLO_J[k]], a[CYCLO_J[k] + 3]
        x2, y2 = f2_sqr(x), f2_sqr(y)
        lo = f2_add(x2, f2_mul_xi(y2))
        hi = f2_sub(f2_sub(f2_sqr(f2_add(x, y)), x2), y2)
        part = (lo, hi, f2_mul_xi(hi))[CYCLO_PART[k]]
        three = f2_add(f2_add(part, part), part)
        two = f2_add(a[k], a[k])
        out.append(f2_add(three, two) if CYCLO_SIGN[k] > 0 else f2_sub(three, two))
    return out


def f12_scale_inv(a, n):
    """a / n0 for n = (n0, 0, 0, 0, 0, 0), n0 in Fp2."""
    i = f2_inv(n[0])
    return [f2_mul(c, i) for c in a]


def f12_pow(a, e):
    r = F12_ONE
    while e:
        if e & 1:
            r = f12_mul(r, a)
        a = f12_sqr(a)
        e >>= 1
    return r


def f12_mul_line(f, line):
    """f * (c0 + c2 w^2 + c3 w^3)."""
    c0, c2, c3 = line
    out = []
    for k in range(6):
        t = f2_mul(f[k], c0)
        t2 = f2_mul(f[(k - 2) % 6], c2)
        t3 = f2_mul(f[(k - 3) % 6], c3)
        t = f2_add(t, f2_mul_xi(t2) if k < 2 else t2)
        out.append(f2_add(t, f2_mul_xi(t3) if k < 3 else t3))
    return out


# ---- op tables -----------------------------------------------------------------------------------------------------
# point steps: slots of one lane pair, each an Fp2 value
SLOT_X, SLOT_Y, SLOT_Z, SLOT_T0, SLOT_L0, SLOT_L2, SLOT_L3, SLOT_F = 0, 1, 2, 3, 9, 10, 11, 12
N_SLOTS = 13
OP_MUL, OP_SQR, OP_ADD, OP_SUB, OP_NEG, OP_MULFP, OP_LD = range(7)
LD_QX, LD_QY, LD_PX, LD_PY = range(4)   # OP_LD sources: the pair's affine inputs (PX, PY: the Fp value in both components)
X, Y, Z = SLOT_X, SLOT_Y, SLOT_Z
T0, T1, T2, T3, T4, T5 = range(SLOT_T0, SLOT_T0 + 6)
L0, L2, L3 = SLOT_L0, SLOT_L2, SLOT_L3

# T = (X : Y : Z) homogeneous on the twist y^2 = x^3 + 4 xi.  Untwist (x, y) -> (x / w^2, y / w^3); a line through untwisted
# points, evaluated at P = (xP, yP) in G1 and scaled by w^3 and by factors from Fp2 (both die in the final exponentiation):
#   tangent at T:      (3 X^3 - 2 Y^2 Z) - (3 X^2 Z xP) w^2 + (2 Y Z^2 yP) w^3
#   chord T, Q=(x2,y2): (u x2 - v y2) - (u xP) w^2 + (v yP) w^3,   u = y2 Z - Y, v = x2 Z - X
# point formulas: dbl-1998-cmo-2 (a = 0) and madd-1998-cmo of the EFD, homogeneous projective: no inversion.
DBL_PROG = [
    (OP_SQR, T0, X, 0), (OP_ADD, T1, T0, T0), (OP_ADD, T0, T1, T0),        # t0 = W = 3 X^2
    (OP_MUL, T1, Y, Z),                                                     # t1 = S = Y Z
    (OP_MUL, T2, T0, X), (OP_MUL, T3, Y, T1), (OP_ADD, T4, T3, T3), (OP_SUB, L0, T2, T4),   # t3 = R = Y S; L0 = W X - 2 R
    (OP_MUL, T2, T0, Z), (OP_LD, T4, LD_PX, 0), (OP_MULFP, T2, T2, T4), (OP_NEG, L2, T2, 0),
    (OP_MUL, T2, T1, Z), (OP_ADD, T2, T2, T2), (OP_LD, T4, LD_PY, 0), (OP_MULFP, L3, T2, T4),
    (OP_MUL, T2, X, T3),                                                    # B = X R
    (OP_ADD, T5, T2, T2), (OP_ADD, T5, T5, T5), (OP_ADD, T2, T5, T5),       # t5 = 4 B, t2 = 8 B
    (OP_SQR, T4, T0, 0), (OP_SUB, T4, T4, T2),                              # t4 = H = W^2 - 8 B
    (OP_MUL, X, T4, T1), (OP_ADD, X, X, X),                                 # X3 = 2 H S
    (OP_SUB, T5, T5, T4), (OP_MUL, T5, T0, T5),                             # W (4 B - H)
    (OP_SQR, T2, T3, 0), (OP_ADD, T2, T2, T2), (OP_ADD, T2, T2, T2), (OP_ADD, T2, T2, T2),
    (OP_SUB, Y, T5, T2),                                                    # Y3 = W (4 B - H) - 8 R^2
    (OP_SQR, T2, T1, 0), (OP_MUL, T2, T2, T1), (OP_ADD, T2, T2, T2), (OP_ADD, T2, T2, T2), (OP_ADD, Z, T2, T2),  # Z3 = 8 S^3
]
ADD_PROG = [
    (OP_LD, T2, LD_QY, 0), (OP_MUL, T0, T2, Z), (OP_SUB, T0, T0, Y),        # t0 = u
    (OP_LD, T3, LD_QX, 0), (OP_MUL, T1, T3, Z), (OP_SUB, T1, T1, X),        # t1 = v
    (OP_MUL, T3, T0, T3), (OP_MUL, T2, T1, T2), (OP_SUB, L0, T3, T2),
    (OP_LD, T2, LD_PX, 0), (OP_MULFP, T2, T0, T2), (OP_NEG, L2, T2, 0),
    (OP_LD, T2, LD_PY, 0), (OP_MULFP, L3, T1, T2),
    (OP_SQR, T2, T0, 0), (OP_SQR, T3, T1, 0), (OP_MUL, T4, T1, T3), (OP_MUL, T3, T3, X),   # uu, vv -> t4 = vvv, t3 = R
    (OP_MUL, T2, T2, Z), (OP_SUB, T2, T2, T4), (OP_SUB, T2, T2, T3), (OP_SUB, T2, T2, T3),  # t2 = A
    (OP_MUL, X, T1, T2),
    (OP_SUB, T3, T3, T2), (OP_MUL, T3, T0, T3), (OP_MUL, T5, T4, Y), (OP_SUB, Y, T3, T5),
    (OP_MUL, Z, T4, Z),
]


def run_point_prog(prog, s, src):
    """s: the lane pair's slots (list of Fp2), src: the four OP_LD sources."""
    for op, d, a, b in prog:
        if op == OP_MUL:
            s[d] = f2_mul(s[a], s[b])
        elif op == OP_SQR:
            s[d] = f2_sqr(s[a])
        elif op == OP_ADD:
            s[d] = f2_add(s[a], s[b])
        elif op == OP_SUB:
            s[d] = f2_sub(s[a], s[b])
        elif op == OP_NEG:
            s[d] = f2_neg(s[a])
        elif op == OP_MULFP:          # component-wise: the kernel's lane-local product
            s[d] = (s[a][0] * s[b][0] % P, s[a][1] * s[b][1] % P)
        elif op == OP_LD:
            s[d] = src[a]
        else:
            raise ValueError(op)


def miller_loop(pairs):
    """prod over the pairs (P in G1, Q on the twist, affine; None = infinity, contributes nothing) of f_{|z|, Q}(P), conjugated
    (z < 0): one accumulator, 63 squarings for the whole group."""
    live = []
    for pt, q in pairs:
        if pt is None or q is None:
            continue
        s = [F2_ZERO] * N_SLOTS
        s[X], s[Y], s[Z] = q[0], q[1], F2_ONE
        live.append((s, (q[0], q[1], (pt[0], pt[0]), (pt[1], pt[1]))))
    f = F12_ONE
    for bit in range(Z_ABS.bit_length() - 2, -1, -1):
        f = f12_sqr(f)
        for s, src in live:
            run_point_prog(DBL_PROG, s, src)
            f = f12_mul_line(f, (s[L0], s[L2], s[L3]))
        if (Z_ABS >> bit) & 1:
            for s, src in live:
                run_point_prog(ADD_PROG, s, src)
                f = f12_mul_line(f, (s[L0], s[L2], s[L3]))
    return f12_conj(f)


# final exponentiation: registers r0 .. r5 hold Fp12 values, the input and the result are r0
FE_MUL, FE_CSQR, FE_CONJ, FE_FROB, FE_INVSCALE = range(5)   # FE_FROB: b = n;  FE_INVSCALE: d = a / (coefficient 0 of b)
N_FE_REGS = 6


def final_exp_program():
    prog = []

    def expz(d, a):                     # d = a^z = conj(a^|z|), d != a, a cyclotomic
        prog.append((FE_CSQR, d, a, 0))
        first = True
        for bit in range(Z_ABS.bit_length() - 2, -1, -1):
            if not first:
                prog.append((FE_CSQR, d, d, 0))
            first = False
            if (Z_ABS >> bit) & 1:
                prog.append((FE_MUL, d, d, a))
        prog.append((FE_CONJ, d, d, 0))

    # easy part: a^-1 = conj(a) B / (a conj(a) B), b = a conj(a) in Fp6, B = b^(p^2) b^(p^4), b B in Fp2
    prog += [(FE_CONJ, 1, 0, 0), (FE_MUL, 2, 0, 1), (FE_FROB, 3, 2, 2), (FE_FROB, 4, 3, 2), (FE_MUL, 3, 3, 4),
             (FE_MUL, 4, 2, 3), (FE_MUL, 2, 1, 3), (FE_INVSCALE, 2, 2, 4),
             (FE_MUL, 0, 1, 2),                                  # a^(p^6 - 1)
             (FE_FROB, 1, 0, 2), (FE_MUL, 0, 1, 0)]              # ... ^(p^2 + 1)
    # hard part: (z - 1)^2 (z + p) (z^2 + p^2 - 1) + 3
    expz(1, 0); prog += [(FE_CONJ, 2, 0, 0), (FE_MUL, 1, 1, 2)]
    expz(2, 1); prog += [(FE_CONJ, 3, 1, 0), (FE_MUL, 2, 2, 3)]
    expz(3, 2); prog += [(FE_FROB, 4, 2, 1), (FE_MUL, 3, 3, 4)]
    expz(4, 3); expz(5, 4)
    prog += [(FE_FROB, 4, 3, 2), (FE_MUL, 5, 5, 4), (FE_CONJ, 4, 3, 0), (FE_MUL, 5, 5, 4),
             (FE_CSQR, 1, 0, 0), (FE_MUL, 1, 1, 0), (FE_MUL, 0, 5, 1)]
    return prog


FE_PROG = final_exp_program()


def final_exp(f):
    r = [f] + [F12_ONE] * (N_FE_REGS - 1)
    for op, d, a, b in FE_PROG:
        if op == FE_MUL:
            r[d] = f12_mul(r[a], r[b])
        elif op == FE_CSQR:
            r[d] = f12_cyclo_sqr(r[a])
        elif op == FE_CONJ:
            r[d] = f12_conj(r[a])
        elif op == FE_FROB:
            r[d] = f12_frob(r[a], b)
        elif op == FE_INVSCALE:
            r[d] = f12_scale_inv(r[a], r[b])
        else:
            raise ValueError(op)
    return r[0]


def pairing_product(pairs):
    """prod e(P_j, Q_j)^3 as a flat Fp12 value."""
    return final_exp(miller_loop(pairs))


def pairing(pt, q):
    return pairing_product([(pt, q)])


def gt_bytes(f):
    """The layout of pe_profile_pairing_gt: c_0.c0, c_0.c1, c_1.c0, ... c_5.c1, each 48 bytes big-endian, plain residues."""
    return b"".join(c.to_bytes(48, "big") for k in range(6) for c in f[k])


# Fp products of one group of n pairs, counted from the tables above as the kernel executes them (per lane; a lane pair
# works on one Fp2 coefficient): point ops MUL = 2, SQR = 1, MULFP = 1; an Fp12 product = 12, a line product = 6,
# a cyclotomic squaring = 3, a Frobenius map = 2.
def fp_products_per_lane(n_pairs):
    cost = {OP_MUL: 2, OP_SQR: 1, OP_MULFP: 1}
    dbl = sum(cost.get(op, 0) for op, *_ in DBL_PROG)
    add = sum(cost.get(op, 0) for op, *_ in ADD_PROG)
    n_dbl = Z_ABS.bit_length() - 1
    n_add = bin(Z_ABS).count("1") - 1
    rounds = -(-n_pairs // 6)
    miller = n_dbl * (12 + rounds * dbl + 6 * n_pairs) + n_add * (rounds * add + 6 * n_pairs)
    fe_cost = {FE_MUL: 12, FE_CSQR: 3, FE_FROB: 2, FE_INVSCALE: 5}
    fe = sum(fe_cost.get(op, 0) for op, *_ in FE_PROG)
    return miller, fe
