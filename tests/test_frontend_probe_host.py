"""The frontend probe of tests/frontend_probe.py, checked on the CPU: that its float64 reference is the reference
project's frontend, that its constants are measurements, and that it sees what the white-noise tests cannot.

* The float64 reference, rounded to fp16, meets the existing criterion (<= 1 fp16 ulp, >= 99.5 % equal) against
  fixture g1_frontend -- outputs of the reference project's own modules.
* KAPPA_REF: the oracle's fp32 arithmetic passes the spectrogram criterion on every probe at KAPPA_REF and fails it
  at KAPPA_REF / 2; oracle.linear_to_mel passes the mel criterion on every probe.
* Three mutants of the float64 reference, each at the largest size the existing white-noise criterion accepts
  (asserted: accepted at that size, rejected at the next), are rejected by the new criteria at KAPPA_GPU:
    (a) filter 59 without its outermost weight (3.5e-5 at bin 220): the mel of sweep row 220 is 58 x its tolerance off
        (every one of the 160 outermost weights, from 2.2e-5 up, gives >= 43 x on its row; white noise accepts 7);
    (b) 2^-19 of frame 2 j + 1 in frame 2 j: 2 onset values outside (row 0, bin 0, where the bin-1 tone's two images
        cancel in the even frame and not in its partner); 2^-17 of it also lifts a silent frame off the floor;
    (c) an error of 2^-20 P in every bin: 56 % of the sweep's values outside (still 46 % at 2^-21, none at 2^-22).
  So the probe is sharper than what exists for all three; for (b) by the least, because a frame 160 samples from
  silence is at most 12 loud and the 1e-3 floor adds in quadrature.
"""
import numpy as np
import pytest
import torch

import frontend_probe as F
from oracle import ppg_oracle as O


class Lab:
    """Float64 spectra of the probes and of the white-noise input, and the oracle's outputs, computed once."""

    def __init__(self):
        self._z, self._oracle = {}, {}

    def audio(self, name):
        return F.white_noise() if name == 'white' else F.probes()[name]

    def z(self, name):
        if name not in self._z:
            self._z[name] = F.spectrum64(self.audio(name))
            self._z[name].setflags(write=False)
        return self._z[name]

    def oracle(self, name):
        """(spec16, mel16) of the fp32 oracle"""
        if name not in self._oracle:
            spec = O.spectrogram(self.audio(name)[:, None])
            self._oracle[name] = (spec.numpy(), O.linear_to_mel(spec).numpy())
        return self._oracle[name]

    def old_accepts(self, Z, basis=None):
        """the existing criterion on the white-noise input, for a frontend that computes Z and uses `basis`"""
        spec16, mel16 = F.render(Z, basis)
        return F.old_criterion(spec16, self.oracle('white')[0]) and F.old_criterion(mel16, self.oracle('white')[1])


@pytest.fixture(scope='module')
def lab():
    return Lab()


def test_probe_signals(lab):
    probes = F.probes()
    assert tuple(probes) == F.PROBES
    assert probes['sweep'].shape == (513, 1600) and probes['two_level'].shape == (16, 1600)
    assert probes['onsets'].shape == (len(F.ONSETS), 160 * 53) and probes['scale'].shape == (10, 160 * 37 + 59)
    for name in ('sweep', 'two_level', 'onsets'):
        assert probes[name].shape[1] % 4 == 0                     # the 16-byte staging path
    assert probes['scale'].shape[1] % 4 != 0
    assert all(float(p.abs().max()) <= 1.0 for p in probes.values())
    # sweep: frames 3 .. 6 of row k are a pure tone at bin k -- 256 there, nothing 3 bins away
    z = np.abs(lab.z('sweep'))
    rows = np.arange(513)
    peak = np.where(rows % 512 == 0, 512.0 * np.abs(np.cos(0.37 * rows)), 256.0)        # (bins 0 and 512 are real: the phase counts)
    assert np.allclose(z[rows, rows, 3:7], peak[:, None], rtol=1e-6)
    far = np.abs(rows[:, None] - rows[None]) >= 3
    assert (z[:, :, 3:7][far] < 1e-5).all()                      # (the fp32 rounding of the samples)
    # onsets: the frames the table calls silent are exactly silent, their neighbour is loud
    z = np.abs(lab.z('onsets')).max(axis=1)                       # (rows, frames)
    assert z.shape == (len(F.ONSETS), 53)
    for row, (silent, loud) in enumerate([(10, 11), (21, 20), (11, 12), (22, 21), (15, 16), (32, 31)]):
        assert z[row, silent] == 0.0 and 5.0 < z[row, loud] < 13.0, (row, z[row, silent], z[row, loud])
    assert z[6, :49].max() == 0.0 and z[6, 52] > 1.5 * z[6, 51] > 0
    # scale: the 1e-5 rows sit at the floor
    assert np.abs(lab.z('scale'))[6:9].max() < 1e-3


def test_reference_pinned_to_fixture(golden):
    g = golden('g1_frontend')
    spec16, mel16 = F.render(F.spectrum64(g['audio'][:, 0]))
    assert spec16.shape == g['spec16'].shape and mel16.shape == g['mel16'].shape
    assert F.old_criterion(spec16, g['spec16']) and F.old_criterion(mel16, g['mel16'])
    mel16 = F.render(F.spectrum64(g['ragged_audio'][:, 0]))[1]
    assert mel16.shape == g['ragged_mel16'].shape
    assert F.old_criterion(mel16, g['ragged_mel16'])


def test_kappa_ref_is_a_measurement(lab):
    needed = {}
    for name in F.PROBES:
        Z, spec16 = lab.z(name), lab.oracle(name)[0]
        assert not F.spec_violations(F.render(Z)[0], Z, 0.0).any()          # the exact result needs no allowance
        needed[name] = F.smallest_kappa(spec16, Z)
        d = F.ulp_diff(spec16, F.render(Z)[0])
        print(f'{name}: the fp32 oracle needs kappa {needed[name]:.2f}; {d.max()} fp16 ulps from float64, {(d == 0).mean():.4f} equal')
        assert not F.spec_violations(spec16, Z, F.KAPPA_REF).any(), name
    assert any(F.spec_violations(lab.oracle(name)[0], lab.z(name), F.KAPPA_REF / 2).any() for name in F.PROBES)
    assert F.KAPPA_REF - 0.1 < max(needed.values()) <= F.KAPPA_REF                 # rounded up to one decimal
    assert F.KAPPA_GPU == 4 * F.KAPPA_REF


@pytest.mark.parametrize('name', F.PROBES)
def test_oracle_mel_passes_the_mel_criterion(lab, name):
    spec16, mel16 = lab.oracle(name)
    worst, equal = F.mel_report(mel16, spec16)
    print(f'{name}: oracle.linear_to_mel worst error {worst:.3f} of the tolerance, {equal:.5f} equal')
    assert F.mel_passes(mel16, spec16)
    # the 1e-5 clamp is out of reach: magnitudes >= 1e-3, every filter's weights sum to >= 0.062
    assert F.basis64().sum(axis=1).min() >= 0.062 and float(spec16.min()) >= 1e-3


def test_mutant_edge(lab):
    """(a) a band table one bin short"""
    filter_index, bin_index = F.MUTANT_EDGE
    weight = float(O.mel_basis()[filter_index, bin_index])
    Zw = lab.z('white')
    assert lab.old_accepts(Zw)
    accepted = [(w, m, b) for w, m, b in F.edge_candidates() if lab.old_accepts(Zw, F.edge_mutant(m, b))]
    print(f'white noise accepts {len(accepted)} of {len(F.edge_candidates())} missing edge weights, the largest {accepted[-1]}')
    assert accepted[-1][1:] == F.MUTANT_EDGE and accepted[-1][0] == weight
    # the sweep row of that bin rejects it -- as the row of every other edge rejects its own
    spec16 = F.render(lab.z('sweep'))[0]
    assert F.mel_passes(F.render(lab.z('sweep'))[1], spec16)
    smallest = np.inf
    for w, m, b in F.edge_candidates():
        mel16 = F.render(lab.z('sweep')[b:b + 1], F.edge_mutant(m, b))[1]
        worst, _ = F.mel_report(mel16, spec16[b:b + 1])
        smallest = min(smallest, worst)
        if (m, b) == F.MUTANT_EDGE:
            print(f'filter {m} without bin {b} (weight {w:.2e}): sweep row {b} is {worst:.0f} x the tolerance off')
            assert worst > 10 and not F.mel_passes(mel16, spec16[b:b + 1])
    print(f'every missing edge weight: >= {smallest:.0f} x the tolerance on its row')
    assert smallest > 10


def test_mutant_crosstalk(lab):
    """(b) the odd frame of a pair leaks into the even one"""
    Zw, eps = lab.z('white'), F.MUTANT_CROSSTALK
    assert lab.old_accepts(F.crosstalk_mutant(Zw, eps)) and not lab.old_accepts(F.crosstalk_mutant(Zw, 2 * eps))
    Z = lab.z('onsets')
    bad = F.spec_violations(F.render(F.crosstalk_mutant(Z, eps))[0], Z, F.KAPPA_GPU)
    print(f'crosstalk 2^{np.log2(eps):.0f}: {bad.sum()} onset values outside, at (row, bin, frame) {np.argwhere(bad)[:4].tolist()}')
    assert bad.any()
    assert not bad[:, :, 1::2].any()                                # only even frames are touched
    # four times as much also lifts the silent even frame of row 0 off the floor
    bad = F.spec_violations(F.render(F.crosstalk_mutant(Z, 4 * eps))[0], Z, F.KAPPA_GPU)
    assert bad[0, :, 10].any()
    # the controls, silent frames whose loud neighbour belongs to another pair, stay on it
    assert not bad[2, :, 11].any() and not bad[3, :, 22].any()


def test_mutant_noise(lab):
    """(c) an error of the size of a sloppy twiddle table in every bin"""
    Zw, eps = lab.z('white'), F.MUTANT_NOISE
    assert lab.old_accepts(F.noise_mutant(Zw, eps)) and not lab.old_accepts(F.noise_mutant(Zw, 2 * eps))
    Z = lab.z('sweep')
    bad = F.spec_violations(F.render(F.noise_mutant(Z, eps))[0], Z, F.KAPPA_GPU)
    print(f'noise 2^{np.log2(eps):.0f}: {bad.mean():.3f} of the sweep outside')
    assert bad.mean() > 0.25
    assert F.spec_violations(F.render(F.noise_mutant(Z, eps / 2))[0], Z, F.KAPPA_GPU).mean() > 0.25
