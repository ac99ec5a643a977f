"""The credibility-interval draws (k_ci_draw with rsem::gamma_draw_bulk, k_ci_scales of ci.hip) replayed value for value on
the CPU by tests/sampler_ref.py: y[j, s] = float32(Gamma(c[s // nSpC, j] + pseudoC; Philox(seed; s, j, 'CIS1')) * w_j),
tpm = float32(y * 1e6 / sum_j y), lbar = float32(sum_j y eel_j / sum_j y).

Bounds (from the number formats, not from what the kernel gives):
  tpm   two float32 roundings separate the double gamma variate from tpm (y, then tpm itself); the device's libm may move
        the double by a few of ITS ulps, which can flip either rounding by one float32 ulp: |d - r| <= 2^-22 |r|, plus one
        float32 denormal step so that 0 == 0 passes; zeros must be zeros on both sides.
  lbar  a float32 quotient of two double sums of the already rounded y: every y within one float32 ulp (2^-23 relative)
        puts each sum -- positive terms -- within 2^-23, the quotient within 2^-22, and the final rounding of the two
        sides adds one float32 ulp: |d - r| <= 3 * 2^-23 |r|.
Only entries whose reference gamma had an accept / reject margin under 1e-9 could be left out; the inputs below have none
(test_ci_replay_inputs_have_no_near_tie asserts it without a GPU: the replay needs nothing from the device).

Largest |difference| / bound seen on an MI355X: 0 for tpm and 0 for lbar in every case -- not one of the 2.9 million tpm
entries differs from the replay's float32 at all (every test prints its own figure).
"""
import numpy as np
import pytest

import sampler_ref as sr

RTOL_TPM = 2.0 ** -22
ATOL_TPM = float(np.finfo(np.float32).smallest_subnormal)
RTOL_LBAR = 3.0 * 2.0 ** -23
NEAR_TIE = 1e-9

# (M, nCV, nSpC): the draw kernel takes the transcripts in chunks of ceil(M / min(M, ceil(8192 / ceil(nS / 64)))) per workgroup
SHAPES = {"chunks of 3, last one short, nS = 40 * 65": (500, 40, 65),     # nS = 2600 = 40 * 64 + 40: a partial last wave
          # "M smaller than one chunk" as far as the kernel's formula allows: chunk = ceil(M / nchunks) <= M, and chunk == M only
          # with a single chunk, i.e. more than 8192 sample blocks of 64 -- hence nS = 524290 (8193 blocks) and a tiny M
          "one chunk holds all of M = 3": (3, 8066, 65),
          "nSpC = 1": (37, 70, 1),                                        # a new count vector in every lane
          "nSpC = 3": (37, 43, 3),                                        # s // nSpC changes inside a wave, 129 = 2 * 64 + 1
          "nSpC = 64": (37, 3, 64)}                                       # ... exactly at the wave's edge
CASES = [(k, p) for k in SHAPES for p in (1.0, 0.3)]


def _inputs(M, nCV, nSpC):
    rng = np.random.default_rng(M * 1000 + nCV)
    cv = rng.choice([0, 0, 1, 1, 2, 17, 1000, 999983, 1000003], (nCV, M + 1)).astype(np.int32)
    omitted = rng.random(M + 1) < 0.1
    omitted[[0, 1]] = False
    cv[:, omitted] = -1                                     # omitted transcripts: -1 in every count vector
    eel = rng.uniform(100.0, 4000.0, M + 1)
    mw = np.where(rng.random(M + 1) < 0.2, 0.85, 1.0)
    z = np.flatnonzero(~omitted)[2:]
    eel[z[::7]] = 0.0                                       # zero weight: no effective length ...
    mw[z[3::11]] = 0.0                                      # ... or not mappable at all
    eel[0] = 0.0
    return cv, eel, mw


_REF = {}


def _reference(shape, pseudoC):
    """(inputs, tpm, lbar) of the replay, once per case; the near-tie cap (zero entries) is checked here, on the CPU alone."""
    if (shape, pseudoC) not in _REF:
        M, nCV, nSpC = SHAPES[shape]
        cv, eel, mw = _inputs(M, nCV, nSpC)
        tpm, lbar, margin = sr.ci_sample(cv, nSpC, eel, mw, pseudoC, seed=0x1234567890 + M)
        n_tie = int((margin < NEAR_TIE).sum())
        print("%s, pseudoC %g: %d draws, smallest decision margin %.3g" % (shape, pseudoC, int(np.isfinite(margin).sum()), margin.min()))
        assert n_tie == 0, "%d reference draws sit within 1e-9 of an accept / reject boundary: choose another seed" % n_tie
        _REF[(shape, pseudoC)] = (cv, eel, mw, tpm, lbar)
    return _REF[(shape, pseudoC)]


@pytest.mark.parametrize("shape,pseudoC", CASES)
def test_ci_replay_inputs_have_no_near_tie(shape, pseudoC):
    """No GPU needed: the committed inputs and seeds give the replay no decision within 1e-9 of its boundary, hold every
    kind of entry the GPU test is about, and the replay's TPM sum to 1e6.  (About 6 million reference draws over the ten
    cases, vectorised: 2.5 s in all, 0.5 s for the largest case.)"""
    M, nCV, nSpC = SHAPES[shape]
    cv, eel, mw, tpm, lbar = _reference(shape, pseudoC)
    assert tpm.shape == (M, nCV * nSpC) and np.all(np.isfinite(tpm)) and np.all(np.isfinite(lbar))
    assert np.allclose(tpm.astype(np.float64).sum(0), 1e6, rtol=1e-5)
    dead = (cv[:, 1:].T < 0) | (eel[1:, None] == 0) | (mw[1:, None] == 0)
    assert np.all(tpm[np.repeat(dead, nSpC, axis=1)] == 0)
    if M > 3:
        assert (cv < 0).any() and (cv == 0).any() and (cv > 900000).any() and (eel[1:] == 0).any() and (mw[1:] == 0).any()
    chunk = -(-M // max(1, min(M, -(-8192 // -(-nCV * nSpC // 64)))))
    if shape.startswith("chunks of 3"):
        assert chunk == 3 and M % chunk != 0 and (nCV * nSpC) % 64 != 0
    if shape.startswith("one chunk"):
        assert chunk == M


@pytest.mark.gpu
@pytest.mark.parametrize("shape,pseudoC", CASES)
def test_ci_draws_replayed_value_for_value(shape, pseudoC):
    from rsem_amd import capi
    M, nCV, nSpC = SHAPES[shape]
    cv, eel, mw, tpm, lbar = _reference(shape, pseudoC)
    d_tpm, d_lbar = capi.ci_sample(cv, nSpC, eel, mw, pseudoC=pseudoC, seed=0x1234567890 + M)
    r64, l64 = tpm.astype(np.float64), lbar.astype(np.float64)
    e_tpm = np.abs(d_tpm.astype(np.float64) - r64)
    b_tpm = RTOL_TPM * np.abs(r64) + ATOL_TPM
    e_lbar = np.abs(d_lbar.astype(np.float64) - l64)
    print("%s, pseudoC %g: largest |difference| / bound: tpm %.3f (%d of %d entries differ at all), lbar %.3f"
          % (shape, pseudoC, (e_tpm / b_tpm).max(), int((e_tpm > 0).sum()), e_tpm.size, (e_lbar / (RTOL_LBAR * l64)).max()))
    assert np.array_equal(d_tpm == 0, tpm == 0), "zeros must be zeros on both sides"
    bad = np.argwhere(e_tpm > b_tpm)
    assert len(bad) == 0, "tpm[%d, %d]: device %r, replay %r (%d entries beyond 2 float32 ulps)" % (
        bad[0][0], bad[0][1], d_tpm[tuple(bad[0])], tpm[tuple(bad[0])], len(bad))
    bad = np.flatnonzero(e_lbar > RTOL_LBAR * l64)
    assert len(bad) == 0, "lbar[%d]: device %r, replay %r" % (bad[0], d_lbar[bad[0]], lbar[bad[0]])
