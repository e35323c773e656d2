"""TEST INFRASTRUCTURE: the systems, slab settings and Boys-seam geometries that pin the launch structure of tf_build_eri (EriBuild in
tf_eri_host.hip.h: plan_slab_size / run_slab, launch_class, launch_generic, teamc_tasks), with their oracle tensors cached per process.
Used by tests/test_eri_shapes.py (CPU) and tests/test_gpu_eri_shapes.py (GPU, and its child processes).  Nothing in the product imports
this module."""
from __future__ import annotations

import math
import os

import numpy as np

import fock_reference as fr
from conftest import make_system
from tuna_amd import molecule as mol

# The Boys function of the ERI and nuclear-attraction kernels (tf_internal.h, team_tables in tf_eri_team.hip.h): below T = 36 a Taylor
# expansion about the nearest point i = (int)(8 T + 0.5) of a grid of step 1/8, rows 0 .. 288; from T = 36 on the asymptotic branch.
BOYS_STEP, BOYS_TMAX = 0.125, 36.0
SEAMS = (0.0625, 0.1875, 17.9375, 35.9375)                    # T at which the grid index rounds up: rows 0|1, 1|2, 143|144, 287|288

TABLE_TAGS = ("n2_ccpvdz", "c2_n2_ccpvtz", "high_l")           # conftest.make_system
TINY_TAGS = ("one_s", "two_s", "one_p", "one_d")               # fock_reference.system: N = 1, 2, 3, 5
SLAB_TAGS = ("n2_ccpvdz", "f_mix", "high_l", "c2_n2_ccpvtz")
CARTESIAN_SLAB_TAGS = ("n2_ccpvdz", "f_mix")
# ten primitives in one p shell: (pp|pp) has 10^4 primitive quartets and Hermite tables of 2 x 100 x 24 doubles per pair, beyond what
# eri_class_kernel stages in LDS -- the one system here that reaches eri_class_kernel<false, false>
DEEP_P_BASIS = {7: [("P", [(0.08 * 1.9 ** k, 0.3 + 0.1 * ((3 * k) % 5)) for k in range(10)])]}


def system(tag):
    """(atoms, shells, aos)"""
    if tag in TABLE_TAGS:
        return make_system(tag)[:3]
    if tag == "deep_p":
        atoms = mol.make_atoms(["N"], None)
        shells = mol.build_shells(atoms, DEEP_P_BASIS)
        return atoms, shells, mol.expand_cartesian_aos(shells)
    if tag.startswith("seam:"):
        return seam_system(float.fromhex(tag[5:]))
    return fr.system(tag)


def seam_tag(R):
    return "seam:" + float(R).hex()


def seam_system(R):
    """Two N centres at distance R; on each one primitive of exponent 1.0 in each of S, P, D, F, G, H and one S primitive of exponent
    0.5: 57 Cartesian AOs per centre.  Exponent-1 pairs have p = 2, so (AA|BB) has alpha = 1, PQ = R, T = R^2; (AA|AB) T = R^2 / 4;
    (AB|AB) T = 0 with R != 0; the nuclear attraction of an exponent-0.5 pair against the other nucleus p = 1, T = R^2."""
    atoms = mol.make_atoms(["N", "N"], float(R))
    table = [(letter, [(1.0, 1.0)]) for letter in "SPDFGH"] + [("S", [(0.5, 1.0)])]
    shells = mol.build_shells(atoms, {7: table})
    return atoms, shells, mol.expand_cartesian_aos(shells)


def _with_neighbours(x):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def seam_distances():
    """The R list: sqrt of the four seams and of 1e-16 with both neighbours; 6 with both neighbours (R^2 = 36); 12 (R^2 / 4 = 36); 0.2,
    30 and 200 (everything between the centres underflows)."""
    out = []
    for t in (1e-16,) + SEAMS:
        out += _with_neighbours(math.sqrt(t))
    out += _with_neighbours(6.0)
    out += [12.0, 0.2, 30.0, 200.0]
    return out


def probe_T(R):
    """T = alpha * PQ * PQ in float64, as the kernels form it, of the probe quartets of seam_system(R):
    {"(AA|BB)": R^2, "(AA|AB)": R^2 / 4, "(AB|AB)": 0, "V(0.5 0.5|B)": R^2}"""
    R = float(R)
    out = {}
    p = q = 2.0                                                # exponent-1 pairs
    alpha = p * q / (p + q)
    for name, Pz, Qz in (("(AA|BB)", 0.0, R), ("(AA|AB)", 0.0, (1.0 * 0.0 + 1.0 * R) / 2.0), ("(AB|AB)", R / 2.0, R / 2.0)):
        PQ = Pz - Qz
        out[name] = alpha * PQ * PQ
    out["V(0.5 0.5|B)"] = 1.0 * (0.0 - R) * (0.0 - R)           # p = 1, P = A, C = B
    return out


def boys_branch(T):
    """("grid", i) or ("asymptotic", None): the branch of the kernels' Boys function"""
    if T < BOYS_TMAX:
        return "grid", int(T * (1.0 / BOYS_STEP) + 0.5)
    return "asymptotic", None


# ---- bra rows and slab settings -----------------------------------------------------------------------------------------------------

def bra_pair_rows(shells):
    """Cartesian bra rows of every shell pair (A >= B, A-major): what a slab of tf_build_eri is measured in"""
    n = [s.n_cart for s in shells]
    return np.asarray([n[a] * n[b] for a in range(len(n)) for b in range(a + 1)], dtype=np.int64)


def total_rows(shells):
    return int(bra_pair_rows(shells).sum())


def largest_pair(shells):
    return int(bra_pair_rows(shells).max())


def r_mid(shells):
    """The middle slab setting: a quarter of the rows, but no less than the largest pair (which a slab always holds whole)"""
    return max(largest_pair(shells), -(-total_rows(shells) // 4))


def n_bra_pairs(shells, rank=0, world=1, spherical=True, layout="packed"):
    """Bra shell pairs of a rank = the slabs of a build with TF_SLAB_ROWS=1"""
    if world == 1:
        return len(shells) * (len(shells) + 1) // 2
    from tuna_amd import distributed as tdist
    return int((tdist.shard_owner(shells, world, spherical, layout) == rank).sum())


def rank_rows(shells, rank, world, spherical=True, layout="packed"):
    from tuna_amd import distributed as tdist
    return int(bra_pair_rows(shells)[tdist.shard_owner(shells, world, spherical, layout) == rank].sum())


def slab_settings(shells):
    """[(name, environment, check of the slab count)]"""
    npairs = n_bra_pairs(shells)
    return [("one slab", {}, lambda n: n == 1),
            ("TF_SLAB_MB=1", {"TF_SLAB_MB": "1"}, lambda n: n >= 1),
            ("TF_SLAB_ROWS=R_mid", {"TF_SLAB_ROWS": str(r_mid(shells))}, lambda n: 3 <= n <= npairs),
            ("TF_SLAB_ROWS=1", {"TF_SLAB_ROWS": "1"}, lambda n: n == npairs)]


def team_class_launches(shells):
    """[(La + Lb, Lc + Ld)] of the class launches of a ONE-slab per-class build of an uncontracted basis of complete shells in the
    packed or tiles layout (EriBuild::run_slab / launch_class): a pair class is (La, Lb); the slab's bra pairs form one run per class;
    a ket class is launched against a run when one of its pairs has a first shell <= the largest first shell of the run"""
    assert all(len(s.exps) == 1 for s in shells)
    first = {}
    for a in range(len(shells)):
        for b in range(a + 1):
            first.setdefault((shells[a].L, shells[b].L), []).append(a)
    return [(sum(bc), sum(kc)) for bc in first for kc in first if min(first[kc]) <= max(first[bc])]


def team_size_instantiated(lab, lcd, team):
    """eri_team_available (tf_eri_team.hip)"""
    mn = (lab + 1) * (lcd + 1)
    mx = (lab // 2 + 1) * ((lab + 1) // 2 + 1) * (lcd // 2 + 1) * ((lcd + 1) // 2 + 1)
    return lab <= 6 and lcd <= 6 and (mn <= 16 if team == 16 else (mn <= 256 if team == 64 else mx > 32))


# ---- oracle tensors, cached per process -----------------------------------------------------------------------------------------------

_ORACLE = {}


def oracle_tensor(tag, spherical):
    """Dense (ij|kl) of the CPU oracle, Cartesian or mapped to the real harmonics.  Cached; at most one seam geometry is kept (114^4
    doubles each)."""
    key = (tag, bool(spherical))
    if key not in _ORACLE:
        from oracle import oracle as orc
        from oracle import scf_oracle as so
        from tuna_amd.spherical import transformation_matrix
        if tag.startswith("seam:"):
            for k in [k for k in _ORACLE if k[0].startswith("seam:") and k[0] != tag]:
                del _ORACLE[k]
        _, shells, aos = system(tag)
        if (tag, False) not in _ORACLE:
            _ORACLE[(tag, False)] = orc.eri(aos, threads=min(16, os.cpu_count() or 1))
        if spherical:
            _ORACLE[key] = so.eri_to_spherical(transformation_matrix([s.L for s in shells]), _ORACLE[(tag, False)])
    return _ORACLE[key]


def drop_oracle(tag):
    for k in [k for k in _ORACLE if k[0] == tag]:
        del _ORACLE[k]


def ao_classes(shells, spherical):
    """x/y parity class (lx & 1) | (ly & 1) << 1 of every output AO: of a real harmonic, the class its Cartesian components share"""
    cart = np.asarray([(lx & 1) | ((ly & 1) << 1) for s in shells for lx, ly, _ in mol.cartesian_components(s.L)], dtype=np.int64)
    if not spherical:
        return cart
    from tuna_amd.spherical import transformation_matrix
    U = transformation_matrix([s.L for s in shells])
    cls = np.empty(U.shape[0], dtype=np.int64)
    for r in range(U.shape[0]):
        members = cart[np.nonzero(U[r])[0]]
        assert len(members) and np.all(members == members[0])
        cls[r] = members[0]
    return cls


def parity_forbidden(shells, spherical):
    """[N,N,N,N] bool: True where the x/y parity rule (class(i) ^ class(j) != class(k) ^ class(l)) makes (ij|kl) exactly zero"""
    return ~fr.allowed_mask(ao_classes(shells, spherical))
