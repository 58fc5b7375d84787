"""The inputs tests/test_viterbi_stream_host.py and tests/test_gpu_viterbi_stream.py share: graphs and synthesised PPGs,
seeded, so that the host test can check on the very inputs of the GPU tests what those rely on (runs that come out
before the flush, a lag well below the forced one)."""
import math

import torch

from ppgs_amd import alignment

import alignment_reference as R

INF = math.inf
FRAMES = 200
EARLY = ('loop', 'random 700')                                 # these give runs out before the flush
WRAP_WINDOW, WRAP_LAG = 128, 64


def random_graph(count, generator, holes=0.2, wide=2, anywhere=True):
    """Degrees 0 .. 6, and `wide` states of degree 255, 254 and then 200 .. 255.  Without `anywhere` a path begins in
    state 0 only, so every path shares its first frames and something commits before the flush."""
    def weights(size):
        values = -5 * torch.rand(size, generator=generator)
        values[torch.rand(size, generator=generator) < holes] = -INF
        return values.tolist()
    arcs = []
    wide = torch.randperm(count, generator=generator)[:wide].tolist()
    for target in range(count):
        degree = int(torch.randint(0, 7, (), generator=generator))
        if wide and target == wide[0]:
            degree = 255
        elif len(wide) > 1 and target == wide[1]:
            degree = 254
        elif target in wide:
            degree = int(torch.randint(200, 256, (), generator=generator))
        sources = torch.randint(0, count, (degree,), generator=generator).tolist()
        arcs += [(source, target, weight) for source, weight in zip(sources, weights(degree))]
    initial = weights(count) if anywhere else [-INF] * count
    initial[0] = -1.                                            # some state may begin, some may end
    final = weights(count)
    final[count - 1] = -1.
    return alignment.graph(torch.randint(0, 40, (count,), generator=generator).tolist(), arcs,
                           stay=weights(count), initial=initial, final=final)


def said(labels, generator, frames=None):
    """(40, T) fp32: a PPG that says the frame labels clearly; padded with silence (39) or cut to `frames`."""
    labels = list(labels)
    if frames is not None:
        labels = (labels + [39] * frames)[:frames]
    logits = torch.randn(40, len(labels), generator=generator)
    logits[torch.tensor(labels), torch.arange(len(labels))] += 12.
    return torch.softmax(logits, dim=0)


def spoken(lexicon, string, generator, pause_every=3):
    """The frame labels of a word string with a pause before it and after every `pause_every`-th word."""
    labels = [39] * 3
    for position, word in enumerate(string):
        for phoneme in lexicon[word][1][0]:
            labels += [phoneme] * int(torch.randint(3, 6, (), generator=generator))
        if position % pause_every == 0:
            labels += [39] * 4
    return labels


def wrap_loop():
    """(graph, lexicon): the ten-word loop, three phonemes a word, no phoneme twice."""
    pool = torch.randperm(39, generator=torch.Generator().manual_seed(5000)).tolist()
    lexicon = [(f'word{w}', [[pool.pop() for _ in range(3)]]) for w in range(10)]
    return alignment.word_loop(lexicon, penalty=1.5)[0], lexicon


def chain(count, generator):
    """`count` phonemes, repeated ones among them, no two neighbours alike."""
    out = [int(torch.randint(0, 39, (), generator=generator))]
    while len(out) < count:
        phoneme = int(torch.randint(0, 39, (), generator=generator))
        if phoneme != out[-1]:
            out.append(phoneme)
    return out


_made = {}


def first_cases():
    """(names, graphs, ppgs (40, FRAMES) each): the batch of the (I1) test."""
    if 'first' not in _made:
        generator = torch.Generator().manual_seed(41800)
        names, graphs, ppgs = [], [], []

        def add(name, graph, ppg):
            names.append(name); graphs.append(graph); ppgs.append(ppg)
        for count in (5, 64, 65, 300):                         # 300: two passes, and no path in 200 frames
            add(f'chain {count}', alignment.chain_graph(chain(count, generator)), R.random_ppg(FRAMES, 3., generator))
        phonemes = chain(40, generator)
        flags = [n % 3 == 1 for n in range(40)]
        add('chain optional', alignment.chain_graph(phonemes, optional=flags), R.random_ppg(FRAMES, 3., generator))
        words = [[chain(4, generator), chain(3, generator)], [chain(5, generator)],
                 [chain(2, generator), chain(4, generator), chain(3, generator)]]
        add('sausage', alignment.pronunciations(words)[0], R.random_ppg(FRAMES, 3., generator))
        loop, lexicon = wrap_loop()
        string = torch.randint(0, 10, (16,), generator=generator).tolist()
        add('loop', loop, said(spoken(lexicon, string, generator), generator, FRAMES))
        add('random 700', random_graph(700, generator, anywhere=False), R.random_ppg(FRAMES, 3., generator))
        add('random 300 wide', random_graph(300, generator, wide=22), R.random_ppg(FRAMES, 3., generator))
        assert int(graphs[-1].offsets[-1]) > 4096              # its arcs come from memory
        _made['first'] = (names, graphs, ppgs)
    return _made['first']


def wrap_case(kind):
    """(graph, ppg (40, T)), T = 300 .. 600: the recordings of the ring test."""
    if kind not in _made:
        generator = torch.Generator().manual_seed(41801)
        loop, lexicon = wrap_loop()
        string = torch.randint(0, 10, (26,), generator=generator).tolist()
        ppg = said(spoken(lexicon, string, generator), generator)
        assert 300 <= ppg.shape[1] <= 600
        graph = loop if kind == 'loop' else alignment.model_graph(alignment.switch_penalty(4.))
        _made[kind] = (graph, ppg)
    return _made[kind]


def random_model(seed):
    """transitions, initial, final with -inf entries that leave a path."""
    generator = torch.Generator().manual_seed(seed)
    A = -5. * torch.rand(40, 40, generator=generator)
    A[torch.rand(40, 40, generator=generator) < 0.3] = -INF
    A.fill_diagonal_(-0.25)
    initial, final = -2. * torch.rand(40, generator=generator), -2. * torch.rand(40, generator=generator)
    initial[torch.rand(40, generator=generator) < 0.3] = -INF
    final[torch.rand(40, generator=generator) < 0.3] = -INF
    return {'transitions': A, 'initial': initial, 'final': final}


def forced_cases():
    """[(label, graph, ppg)]: a 40-phoneme chain, a 300-state chain and a sausage, each said clearly."""
    if 'forced' not in _made:
        generator = torch.Generator().manual_seed(41802)
        out = []
        for count in (40, 300):
            phonemes = chain(count, generator)
            low = 4 if count == 40 else 1                      # 200 to 600 frames either way
            labels = [p for p in phonemes for _ in range(int(torch.randint(low, 2 * low + 1, (), generator=generator)))]
            out.append((f'chain {count}', alignment.chain_graph(phonemes), said(labels, generator)))
        words = [[chain(4, generator), chain(3, generator)], [chain(5, generator)],
                 [chain(2, generator), chain(4, generator), chain(3, generator)]]
        labels = [39] * 5
        for variants in words:
            choice = variants[int(torch.randint(0, len(variants), (), generator=generator))]
            labels += [p for p in choice for _ in range(int(torch.randint(4, 9, (), generator=generator)))] + [39] * 6
        labels = (labels * 4)[:230]                             # the words once, then frames no path explains well
        out.append(('sausage', alignment.pronunciations(words)[0], said(labels, generator)))
        assert all(200 <= ppg.shape[1] <= 600 for _, _, ppg in out)
        _made['forced'] = out
    return _made['forced']


def ragged_case():
    """(graphs of 3, 65 and 300 states, ppg (3, 40, 150))."""
    if 'ragged' not in _made:
        generator = torch.Generator().manual_seed(41803)
        graphs = [alignment.chain_graph(chain(3, generator)), alignment.chain_graph(chain(65, generator)),
                  random_graph(300, generator)]
        ppg = torch.stack([R.random_ppg(150, scale, generator) for scale in (1., 3., 8.)])
        _made['ragged'] = (graphs, ppg)
    return _made['ragged']


def _replace(packed, **fields):
    return packed._replace(**fields)


def _bad_source(packed):
    sources = packed.sources.clone()
    sources[0] = 3                                             # graph 0 has states 0 .. 2
    return _replace(packed, sources=sources)


def _bad_degree(packed):
    """255 more arcs into state 1 of graph 0: a degree of 256."""
    extra = 255
    sources = torch.cat([packed.sources[:1], torch.zeros(extra, dtype=torch.int32, device=packed.sources.device),
                         packed.sources[1:]])
    weights = torch.cat([packed.weights[:1], torch.zeros(extra, dtype=torch.float32, device=packed.weights.device),
                         packed.weights[1:]])
    arc_begin = packed.arc_begin.clone()
    arc_begin[2:] += extra
    return _replace(packed, arcs=packed.arcs + extra, sources=sources.contiguous(), weights=weights.contiguous(),
                    arc_begin=arc_begin)


def _bad_weight(packed):
    stay = packed.stay.clone()
    stay[0] = math.nan
    return _replace(packed, stay=stay)


# what makes the device refuse graph 0 of a PackedGraphs whose first graph has three states and the arcs 0 -> 1 -> 2
DAMAGE = {'a source out of range': _bad_source, 'a degree of 256': _bad_degree, 'a NaN weight': _bad_weight,
          'which_graph out of range': lambda packed: packed}
