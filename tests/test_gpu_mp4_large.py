"""GPU: MP4(SDQ) of tf_mp4_rhf at the sizes where the ladder kernel's loops run more than once -- synth-400 with the orbitals of the bench
leg (o = 18, and 10 frozen) and synth-200 on the three layouts.  No dense tensor fits, so, as in tests/test_gpu_mp3_large.py:
  * E_D and E_Q against the step differences of tf_ccd_rhf (E[LCCD step 2] - E[LCCD step 1], E[CCD step 1] - E[LCCD step 1]; its update
    kernel and intermediates, which tests/test_gpu_ccd_large.py pins at this size);
  * E_S against tests/mp4_reference.py's closed-shell form from (ia|jb) and (ki|ld) of tf_ao_to_mo and Z[T] = K[T^T] of the general-density
    exchange build: no MP4 code of the library takes part.
Bound |d| <= 1e-10 S, the project's bound at synth-400.  For the singles S is the reference's own sum of magnitudes.  For E_D and E_Q it is
S = sum |w_ijab dt_ijab|, w = 2 (ia|jb) - (ib|ja), dt = the difference of the two steps' amplitudes: dt = (Q_ijab + Q_jiba) / D, so by the
triangle inequality this S is at most sum |t' Q| -- the bound asks no less than the one with sum |t' Q|.
Every test hands the shared context back with the default layout."""
import os
import re
import time

import numpy as np
import pytest

import mp4_reference as m4
from test_gpu_ccd_large import _converged_orbitals
from test_gpu_mp2_large import _reset, _synthetic, bench_orbitals  # noqa: F401  (bench_orbitals: a fixture)
from test_gpu_mp3_large import _Z_from_exchange

pytestmark = pytest.mark.gpu

TFL_W = 64                                    # pairs of a batch of the ladder stage (tf_mp3.hip.h): the occupied rows are made per batch
SINGLES_THREADS = 256                         # threads of mp4_singles_kernel's workgroup, one workgroup per (i, a)
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tuna_amd", "csrc")


def _batches(o):
    return [min(TFL_W, o * o - p0) for p0 in range(0, o * o, TFL_W)]


def test_mirror_of_the_singles_path_constants():
    """The singles path adds no slicing of its own: the occupied rows are back-transformed per batch of TFL_W pairs of the ladder stage
    (work space TFL_W N o), and mp4_singles_kernel walks o^2 v products per (i, a) with SINGLES_THREADS threads.  If one of these changes
    in the library, this test fails instead of the others silently missing the edge."""
    mp3, mp4, dev = (open(os.path.join(CSRC, f)).read() for f in ("tf_mp3.hip.h", "tf_mp4.hip.h", "tf_corr_host.hip.h"))
    assert int(re.search(r"#define TFL_W (\d+)", mp3).group(1)) == TFL_W
    assert re.search(r"__shared__ double s_u\[(\d+)\], s_r\[(\d+)\];", mp4).groups() == (str(SINGLES_THREADS),) * 2
    assert re.search(r"mp4_singles_kernel, dim3\(\(unsigned\)ov\), dim3\((\d+)\)", dev).group(1) == str(SINGLES_THREADS)
    assert "(size_t)TFL_W * N * o" in dev
    # the edges the tests below reach
    assert _batches(18) == [64] * 5 + [4] and _batches(8) == [64]
    for o, v in ((18, 382), (8, 382), (18, 182)):
        assert o * o * v > SINGLES_THREADS                           # every thread of a workgroup has work, several passes
        assert (o * o * v) % SINGLES_THREADS != 0                    # and the last pass is partial


def _singles_inputs(eng, C, eps, o):
    """occupied_rows and (ki|ld) of the full window [0, o); a frozen core is a slice"""
    Co, Cv = np.ascontiguousarray(C[:, :o]), np.ascontiguousarray(C[:, o:])
    ovov = eng.ao_to_mo(Co, Cv, Co, Cv)
    q = eng.ao_to_mo(Co, Co, Co, Cv)
    t, OV = m4.occupied_rows(ovov, lambda T: _Z_from_exchange(eng, T), Co, Cv, eps[:o], eps[o:])
    return ovov, q, t, OV


def _check(eng, C, eps, o, nf, inputs, label, bad):
    ovov, q, t, OV = inputs
    ES_ref, S_S = m4.singles_from_rows(t[nf:, nf:], OV[nf:, nf:, nf:], q[nf:, nf:, nf:], eps[nf:o], eps[o:])
    r = eng.mp4_rhf(C, eps, o, nf)
    r3 = eng.mp3_rhf(C, eps, o, nf)
    kw = dict(use_diis=False, conv_delta_E=0.0, conv_amplitudes=0.0, return_t2=True, allow_unconverged=True)
    l1 = eng.ccd_rhf(C, eps, o, nf, method="LCCD", max_iter=1, **kw)
    l2 = eng.ccd_rhf(C, eps, o, nf, method="LCCD", max_iter=2, **kw)
    c1 = eng.ccd_rhf(C, eps, o, nf, method="CCD", max_iter=1, **kw)
    g = ovov[nf:, :, nf:, :]
    w = (2.0 * g - g.transpose(0, 3, 2, 1)).transpose(0, 2, 1, 3)
    ED_ref, EQ_ref = l2["table"][1, 1] - l1["table"][0, 1], c1["table"][0, 1] - l1["table"][0, 1]
    S_D, S_Q = float(np.sum(np.abs(w * (l2["t2"] - l1["t2"])))), float(np.sum(np.abs(w * (c1["t2"] - l1["t2"]))))
    for name, ref, S in (("E_S", ES_ref, S_S), ("E_D", ED_ref, S_D), ("E_Q", EQ_ref, S_Q)):
        err = abs(r[name] - ref)
        print(f"[{label}, {nf} frozen] {name} {r[name]:.12e} ref {ref:.12e} |d| {err:.2e} |d|/S {err / S:.2e} (S {S:.3e})")
        if not err <= 1e-10 * S:
            bad.append(f"{label}, {nf} frozen: {name} = {r[name]!r}, reference {ref!r}, |d|/S = {err / S:.2e}")
    if not all(r[k] == r3[k] for k in ("E_OS", "E_SS", "E_pp", "E_hh", "E_ring")):
        bad.append(f"{label}, {nf} frozen: the MP2 / MP3 parts of tf_mp4_rhf are not bit for bit those of tf_mp3_rhf: {r} {r3}")
    dq = eng.mp4_rhf(C, eps, o, nf, level="DQ")
    if not (dq["E_S"] == 0.0 and dq["E_D"] == r["E_D"] and dq["E_Q"] == r["E_Q"]):
        bad.append(f"{label}, {nf} frozen: DQ {dq} against SDQ {r}")
    print(f"[{label}, {nf} frozen] seconds MP4 {r['seconds']} MP3 {r3['seconds']}")
    return r


def test_components_at_400_bench_orbitals_and_frozen_core(engine, bench_orbitals):
    """synth-400, the converged orbitals of the bench leg, o = 18 (324 pairs: five full batches and one of 4); 10 frozen (o = 8: exactly one
    full batch of 64 pairs)"""
    t0 = time.perf_counter()
    aos, C, eps, o = bench_orbitals
    try:
        engine.set_basis(aos).build_eri(True)
        assert engine.eri_storage()["layout"] == "packed" and engine.N == 400 and o == 18
        inputs = _singles_inputs(engine, C, eps, o)
        t1 = time.perf_counter()
        bad, got = [], {}
        print()
        for nf in (0, 10):
            got[nf] = _check(engine, C, eps, o, nf, inputs, "synth-400 bench orbitals", bad)
        print(f"[synth-400 bench orbitals] reference inputs {t1 - t0:.1f} s, the rest {time.perf_counter() - t1:.1f} s")
        assert not bad, "\n".join(bad)
        assert abs(got[10]["E_MP4"] - got[0]["E_MP4"]) > 1e-7           # (the frozen orbitals did leave)
    finally:
        _reset(engine)


def test_components_at_200_on_every_layout(engine):
    """synth-200, converged RHF orbitals, o = 18, on packed, tiles and rows: the ladder kernel with both stored-triangle halves of the
    occupied rows, and the exchange-build route on the other two layouts"""
    bad = []
    try:
        aos, C, eps, o = _converged_orbitals(engine, 200)
        inputs = _singles_inputs(engine, C, eps, o)
        print()
        for layout in ("packed", "tiles", "rows"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == 200
            _check(engine, C, eps, o, 0, inputs, f"synth-200 {layout}", bad)
    finally:
        _reset(engine)
    assert not bad, "\n".join(bad)
