"""Frame metrics, host side (no GPU): the C ABI of ppg_metrics_*, the result formatting of
ppgs_amd.evaluate.Metrics, the float64 restatement the GPU tests use (pinned here to the reference's own
accumulators, fixture g13), and the ISA audit of the built metrics kernel."""
import ctypes
import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-5, 2e-6          # per frame: the bound of test_postops_match_reference_fixture for this arithmetic
FIXED = 2.0 ** -32


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def case_inputs(g, case):
    """(logits, labels, lengths) of a fixture case; B is regenerated from its seed and checked"""
    if case != 'B':
        return (torch.from_numpy(g[f'{case}_logits']), torch.from_numpy(g[f'{case}_labels']),
                torch.from_numpy(g[f'{case}_lengths']))
    generator = _tool('make_golden_metrics')
    logits, labels, lengths = generator.build_inputs(int(g['B_seed']), *generator.CASES['B'])
    assert generator.checksums(logits) == (float(g['B_checksum']), float(g['B_abs_checksum'])), \
        'torch.randn no longer reproduces case B'
    assert torch.equal(lengths, torch.from_numpy(g['B_lengths']))
    return logits, labels, lengths


def restate(logits, labels, lengths=None, k=3, mix=None, class_weights=None, loss_weights=None,
            loss_clamp=2.0 ** 20):
    """The seven accumulators in float64 torch (integers exact: comparisons of the fp32 logits themselves).
    A frame's loss is brought into [0, loss_clamp] as the header states (None: left as it is); labels that are
    neither -100 nor a class are counted in `invalid_labels` and ignored; `topk_by_k[j - 1]` is topk_correct at
    k = j for every accepted k."""
    batch, classes, frames = logits.shape
    labels = labels.to(torch.int64).clone()
    if lengths is not None:
        labels[torch.arange(frames)[None, :] >= torch.as_tensor(lengths)[:, None]] = -100
    keep = labels.flatten() != -100
    invalid = int((keep & ((labels.flatten() < 0) | (labels.flatten() >= classes))).sum())
    keep = keep & (labels.flatten() >= 0) & (labels.flatten() < classes)
    rows = logits.float().transpose(1, 2).flatten(0, 1)[keep]
    target = labels.flatten()[keep]
    n = int(keep.sum())
    order = torch.sort(rows, dim=1, descending=True, stable=True).indices      # ties: lowest index first
    correct = order[:, 0] == target
    probs = torch.softmax(rows.double(), dim=1)
    onehot = torch.nn.functional.one_hot(target, classes).double()
    nll = -torch.log_softmax(rows.double(), dim=1).gather(1, target[:, None])[:, 0]
    if loss_weights is not None:
        nll = nll * loss_weights.double()[target]
    if loss_clamp is not None:
        nll = nll.clamp(0., loss_clamp)
    x, y = probs.clamp(1e-8, 1 - 1e-8).T, onehot.clamp(1e-8, 1 - 1e-8).T
    if mix is not None:
        x, y = mix.double() @ x, mix.double() @ y
    log_m = torch.log((x + y) / 2)
    kl = (x * (torch.log(x) - log_m) + y * (torch.log(y) - log_m)) / 2
    jsd = torch.sqrt(kl.clamp(min=0)).sum(dim=0)
    weighted = probs if class_weights is None else probs * class_weights.double()[None]
    predicted = weighted.argmax(dim=1) if n else torch.zeros(0, dtype=torch.int64)
    return dict(
        count=n, true_positives=int(correct.sum()),
        topk_correct=int((order[:, :k] == target[:, None]).sum()), invalid_labels=invalid,
        topk_by_k=np.array([int((order[:, :j] == target[:, None]).sum()) for j in range(1, 9)]),
        class_total=torch.bincount(target[correct], minlength=classes).numpy(),
        class_count=torch.bincount(target, minlength=classes).numpy(),
        loss_sum=float(nll.sum()), jsd_sum=float(jsd.sum()),
        loss_weight_sum=float(loss_weights.double()[target].sum()) if loss_weights is not None else 0.,
        distance_matrix=torch.zeros(classes, classes, dtype=torch.float64).index_add_(0, predicted, weighted).numpy(),
        distance_rows=torch.bincount(predicted, minlength=classes).numpy(),
        confusion=torch.zeros(classes, classes, dtype=torch.float64).index_add_(0, target, probs).numpy())


def mix_of(g):
    return torch.from_numpy(g['similarity']).float().T ** float(g['exponent'])


def check_against_fixture(got, g, case, normalize=True, balanced=False, fixed_point=False):
    """`got`: accumulators as real numbers (restate(), or a state read with the fixed-point fields scaled)."""
    n = int(g[f'{case}_count'])
    for key in ('count', 'true_positives', 'topk_correct'):
        assert got[key] == int(g[f'{case}_{key}']), (case, key)
    for key in ('class_total', 'class_count'):
        assert np.array_equal(np.asarray(got[key]), g[f'{case}_{key}']), (case, key)
    quantum = FIXED if fixed_point else 0.
    expected_loss = float(g[f'{case}_loss_balanced_total' if balanced else f'{case}_loss_total'])
    expected_jsd = float(g[f'{case}_jsd_total' if normalize else f'{case}_jsd_plain_total'])
    for name, value, expected in (('loss', got['loss_sum'], expected_loss), ('jsd', got['jsd_sum'], expected_jsd)):
        if n == 0:
            assert value == 0 and expected == 0, (case, name)
            continue
        print(f'{case} {name}: mean {value / n:.9g} reference {expected / n:.9g} '
              f'relative {abs(value - expected) / max(abs(expected), 1e-30):.3e}')
        assert abs(value / n - expected / n) <= ATOL + RTOL * abs(expected / n) + quantum, (case, name, value, expected)
    counts = g[f'{case}_class_count'].astype(np.float64)
    confusion_bound = ATOL * counts[:, None] + n * quantum + RTOL * np.abs(g[f'{case}_confusion'])
    error = np.abs(got['confusion'] - g[f'{case}_confusion'])
    print(f'{case} confusion: largest error {error.max():.3e}')
    assert (error <= confusion_bound).all(), (case, 'confusion', error.max())
    expected = g[f'{case}_distance_matrix'].astype(np.float64)
    if case == 'B':          # near ties of the weighted argmax may fall either way there: the total only
        total, want = got['distance_matrix'].sum(), expected.sum()
        print(f'B distance matrix total: {total:.9g} reference {want:.9g}')
        assert abs(total - want) <= ATOL * n + RTOL * abs(want) + n * quantum
        return
    rows = np.minimum(counts, got.get('distance_rows', counts).astype(np.float64))
    error = np.abs(got['distance_matrix'] - expected)
    print(f'{case} distance matrix: largest error {error.max():.3e} (largest cell {expected.max():.3e})')
    assert (error <= ATOL * rows[:, None] + n * quantum + RTOL * np.abs(expected)).all(), (case, error.max())


@pytest.mark.parametrize('case', ['A', 'B', 'C', 'D'])
def test_float64_restatement_agrees_with_the_reference_accumulators(golden, case):
    g = golden('g13_metrics')
    logits, labels, _ = case_inputs(g, case)
    weights = torch.from_numpy(g['weights'])
    check_against_fixture(restate(logits, labels, mix=mix_of(g), class_weights=weights), g, case)
    check_against_fixture(restate(logits, labels, class_weights=weights, loss_weights=weights), g, case,
                          normalize=False, balanced=True)


def test_fixture_meets_its_input_conditions(golden):
    g = golden('g13_metrics')
    cases = json.loads(str(g['cases']))
    assert cases['A']['weighted_gap'] >= 1e-3
    assert all(cases[case]['logit_gap'] > 0 for case in 'ABD')
    assert (g['A_labels'] == 39).any() and g['A_class_count'][39] > 0 and g['B_class_count'][39] > 0
    assert int(g['C_count']) == 0 and int(g['D_count']) == 1


def test_state_struct_matches_the_library_and_entry_points_fail_loudly():
    lib = E.library()
    assert ctypes.sizeof(E.PpgMetricsState) == lib.ppg_metrics_state_bytes() == (8 + 2 * 40 + 2 * 1600) * 8
    assert E.PpgMetricsState.class_total.offset == 64 and E.PpgMetricsState.confusion.offset == (8 + 80 + 1600) * 8
    dummy = ctypes.c_void_p(16)

    def update(logits=dummy, labels=dummy, state=dummy, k=3, batch=1, frames=10):
        return lib.ppg_metrics_update(0, logits, labels, 1, None, batch, frames, k, None, None, None, state, None)
    for bad in (dict(k=0), dict(k=9), dict(logits=None), dict(labels=None), dict(state=None), dict(batch=-1),
                dict(state=ctypes.c_void_p(20))):
        assert update(**bad) == -1, bad
    assert lib.ppg_metrics_reset(0, None, None) == -1
    if torch.cuda.is_available():
        return
    assert update() == -2 and b'no HIP device' in lib.ppg_last_error()
    assert lib.ppg_metrics_reset(0, dummy, None) == -2 and b'no HIP device' in lib.ppg_last_error()
    with pytest.raises(E.PpgError):
        E.MetricsState(0)
    with pytest.raises(E.PpgError):
        ppgs_amd.evaluate.Metrics(normalize=False)


def state_dict_from(values, k=3):
    """a MetricsState.read() dict from real-valued accumulators"""
    def fixed(v):
        return np.rint(np.asarray(v, dtype=np.float64) * 2.0 ** 32).astype(np.int64)
    return dict(
        count=values['count'], true_positives=values['true_positives'], topk_correct=values['topk_correct'],
        invalid_labels=0, loss_sum=int(fixed(values['loss_sum'])), loss_weight_sum=0,
        jsd_sum=int(fixed(values['jsd_sum'])), class_total=np.asarray(values['class_total'], dtype=np.int64),
        class_count=np.asarray(values['class_count'], dtype=np.int64),
        distance_matrix=fixed(values['distance_matrix']), confusion=fixed(values['confusion']), k=k)


def test_result_formatting_has_the_reference_keys_and_values(golden):
    g = golden('g13_metrics')
    for case in 'ACD':
        logits, labels, _ = case_inputs(g, case)
        values = restate(logits, labels, mix=mix_of(g), class_weights=torch.from_numpy(g['weights']))
        reference = json.loads(str(g[f'{case}_results']))
        results = ppgs_amd.evaluate.format_results(state_dict_from(values))
        assert list(results) == list(reference)                  # the same keys in the same order
        assert 'Top-3 Accuracy/' in results and 'Accuracy/aa' in results
        for key, expected in reference.items():
            if isinstance(expected, float) and math.isnan(expected):
                assert math.isnan(results[key]), (case, key)
            elif key.startswith(('Total/', 'Count/')):
                assert results[key] == expected and isinstance(results[key], int), (case, key)
            else:
                assert results[key] == pytest.approx(expected, rel=RTOL, abs=ATOL), (case, key)
    figures = ppgs_amd.evaluate.format_results(state_dict_from(values), include_figures=True)
    assert set(figures) - set(results) == {'DistanceMatrix', 'ConfusionMatrix'}
    assert tuple(figures['DistanceMatrix'].shape) == (40, 40)
    values = restate(*case_inputs(g, 'A')[:2])
    figures = ppgs_amd.evaluate.format_results(state_dict_from(values), include_figures=True)
    assert torch.allclose(figures['DistanceMatrix'].sum(dim=1), torch.ones(40, dtype=torch.float64))
    assert 'Top-5 Accuracy/' in ppgs_amd.evaluate.format_results(state_dict_from(values, k=5))
    broken = dict(state_dict_from(values), invalid_labels=2)
    with pytest.raises(ValueError):
        ppgs_amd.evaluate.format_results(broken)


def test_merge_and_fields_are_integer_exact():
    words = np.arange(ctypes.sizeof(E.PpgMetricsState) // 8, dtype=np.int64)
    fields = E.metrics_fields(words)
    assert fields['count'] == 0 and fields['jsd_sum'] == 6 and 'reserved' not in fields
    assert fields['class_total'][0] == 8 and fields['class_count'][0] == 48
    assert fields['distance_matrix'][1, 2] == 88 + 42 and fields['confusion'][0, 0] == 88 + 1600
    fields['k'] = 3
    merged = E.MetricsState.merge(fields, fields, fields)
    assert merged['jsd_sum'] == 18 and merged['confusion'][39, 39] == 3 * (words[-1])
    with pytest.raises(ValueError):
        E.MetricsState.merge(fields, dict(fields, k=4))


def test_save_writes_the_reference_file_names(tmp_path):
    results = {'aggregate': {'Accuracy': 0.5, 'Top-3 Accuracy/': 0.75, 'DistanceMatrix': torch.eye(40)},
               'loss': 1.25}
    ppgs_amd.evaluate.save(results, 'overall', tmp_path)
    assert json.load(open(tmp_path / 'overall.json')) == {
        'aggregate': {'Accuracy': 0.5, 'Top-3 Accuracy/': 0.75}, 'loss': 1.25}
    assert torch.equal(torch.load(tmp_path / 'overall' / 'DistanceMatrix.pt'), torch.eye(40))


def test_phoneme_weights_come_from_the_environment(tmp_path, monkeypatch, golden):
    monkeypatch.delenv('PPGS_AMD_PHONEME_WEIGHTS', raising=False)
    with pytest.raises(ValueError):
        ppgs_amd.evaluate.phoneme_weights()
    path = tmp_path / 'weights.pt'
    torch.save(torch.from_numpy(golden('g13_metrics')['weights']), path)
    monkeypatch.setenv('PPGS_AMD_PHONEME_WEIGHTS', str(path))
    assert tuple(ppgs_amd.evaluate.phoneme_weights().shape) == (40,)


def test_metrics_kernel_isa_has_only_vector_stores_and_atomics():
    """The built library's metrics kernel: 64-bit LDS adds and global vector atomics, no compare-and-swap loop, no
    scratch, and none of the scalar-memory write instructions; the packed-fp32 audit still passes over it."""
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    library = os.path.join(ROOT, 'ppgs_amd', 'libppgs_amd.so')
    if not os.path.exists(objdump):
        pytest.skip('no llvm-objdump')
    if not os.path.exists(library):
        pytest.skip('library not built')
    import glob
    import shutil
    import tempfile
    body = None
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(library, os.path.join(tmp, 'lib.so'))
        subprocess.run([objdump, '--offloading', 'lib.so'], check=True, cwd=tmp, capture_output=True)
        for obj in glob.glob(os.path.join(tmp, '*gfx950*')):
            listing = subprocess.run([objdump, '-d', obj], check=True, capture_output=True, text=True).stdout
            found = re.search(r'<_ZN\S*metrics_kernel\S*>:\n(.*?)(?=\n[0-9a-f]+ <|\Z)', listing, re.S)
            if found:
                body = found.group(1)
    assert body, 'metrics_kernel is not in the built library'
    mnemonics = set(re.findall(r'^\s*([a-z][a-z0-9_]+)', body, re.M))
    scalar, sep = 's', '_'
    banned = [scalar + sep + stem for stem in (
        'store', 'buffer' + sep + 'store', 'scratch' + sep + 'store', 'atomic', 'buffer' + sep + 'atomic',
        'dcache' + sep + 'wb', 'dcache' + sep + 'discard')]
    assert not [m for m in mnemonics if m.startswith(tuple(banned))]
    assert 'global_atomic_add_x2' in mnemonics and 'ds_add_u64' in mnemonics
    assert not [m for m in mnemonics if 'cmpswap' in m or m.startswith('scratch_')]
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pk_scan.py'), '--strict'],
                         capture_output=True, text=True)
    assert run.returncode == 0 and ' 0 exposed' in run.stdout, run.stdout[-2000:]
