"""The inputs the posterior tests share (tests/test_posterior_host.py, tests/test_gpu_posterior.py): random graphs and
PPGs by seed, the tolerance B(T) of the GPU tests, and the sensitivity probe that keeps that tolerance honest.

The tolerance (tests/test_gpu_posterior.py states where it comes from): with M = 18.43 + the largest finite |weight|
of the case (18.43 = -log(1e-8), the largest emission) and d its largest in-degree or out-degree,
    B(T) = (T + 1) * 2**-23 * (4 M + d / 2 + 4)."""
import math

import numpy as np
import torch

import posterior_reference as reference
from ppgs_amd import alignment

# (states, frames, seed) of the random graphs run on the GPU; the seeds were chosen so that the sensitivity condition of
# tests/test_posterior_host.py holds (a dropped arc moves `total` by at least 100 bounds in three cases of four)
RANDOM_CASES = ((3, 5, 21), (64, 97, 10), (65, 129, 7), (700, 64, 13))


def random_ppg(seed, frames, sharpness=3.):
    """A (40, frames) float32 PPG: the softmax of `sharpness` * normal logits."""
    generator = torch.Generator().manual_seed(seed)
    return torch.softmax(sharpness * torch.randn(40, frames, generator=generator), dim=0).float()


def random_graph(seed, count, big=True, most=6):
    """A Graph of `count` >= 3 states: in-degrees 0 .. `most` with sources drawn at random (parallel arcs and arcs n -> n among
    them), weights in [-5, 0] with 30 % of them -inf (stay, initial and final too; state 0 may always begin and the last
    state end); with `big`, one state of in-degree 255 and one whose out-degree is at least 300."""
    rng = np.random.default_rng(seed)

    def weight():
        return -math.inf if rng.random() < 0.3 else float(-5. * rng.random())
    arcs = []
    high = int(rng.integers(count)) if big else -1
    for n in range(count):
        for _ in range(255 if n == high else int(rng.integers(0, most + 1))):
            arcs.append((int(rng.integers(count)), n, weight()))
    if big:
        wide = int(rng.integers(count))
        others = [n for n in range(count) if n != high]       # (count >= 3: at most 150 + 6 more into any of them)
        for j in range(300):
            arcs.append((wide, others[j % len(others)], weight()))
    stay = [weight() for _ in range(count)]
    initial = [weight() for _ in range(count)]
    final = [weight() for _ in range(count)]
    initial[0] = -1.
    final[count - 1] = -.5
    return alignment.graph([int(p) for p in rng.integers(0, 40, count)], arcs, stay, initial, final)


def magnitudes(graph):
    """(M, d) of a Graph for the bound: 18.43 + its largest finite |weight|, and its largest in- or out-degree."""
    values = torch.cat([graph.stay, graph.weights, graph.initial, graph.final]).double()
    finite = values[torch.isfinite(values)]
    largest = float(finite.abs().max()) if finite.numel() else 0.
    offsets = graph.offsets.long()
    degree = int((offsets[1:] - offsets[:-1]).max()) if graph.sources.numel() else 0
    if graph.sources.numel():
        degree = max(degree, int(torch.bincount(graph.sources.long()).max()))
    return 18.43 + largest, degree


def bound(graph, frames):
    """B(T) of the module's text."""
    m, d = magnitudes(graph)
    return (frames + 1) * 2. ** -23 * (4. * m + d / 2. + 4.)


def without_an_arc(graph, gamma):
    """`graph` as Lists without the last finite in-arc of the most occupied state (by the sum of `gamma` over the frames)
    that has one; None if no state has a finite in-arc."""
    g = reference.lists(graph)
    for n in np.argsort(-gamma.sum(axis=0), kind='stable'):
        finite = [j for j, (_, w) in enumerate(g.into[n]) if w > -math.inf]
        if finite:
            into = [list(v) for v in g.into]
            del into[n][finite[-1]]
            return g._replace(into=into)
    return None
