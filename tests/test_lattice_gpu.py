"""GPU: connected-word lattices (csrc/connected_lattice.hip) through the Python layer against the CPU restatement
tests/_lattice_ref.py, which is the definition.  The three kernels are float64 adds, one subtract and strict compares
only, so every comparison to the restatement is ``np.array_equal``.  tests/test_lattice_cpu.py guards, on the CPU, what
these tests rely on: on every random case the best string is unique by more than 1e-6."""
import numpy as np
import pytest

from sapr_amd.connected import connected_lattice
from tests import _bigram_ref as bref
from tests import _lattice_cases as lc
from tests import _lattice_ref as lref

pytestmark = pytest.mark.gpu

NEG = -np.inf
LENGTHS = lc.LENGTHS
BACK = ("beta", "next_end", "next_word", "root", "first")


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


def _assert_forward(lat, tabs, what):
    X, N, B = lat.tables()
    assert np.array_equal(X, tabs["X"]), (what, "X")
    assert np.array_equal(N, tabs["N"]), (what, "N")
    assert np.array_equal(B, tabs["B"]) and B.dtype == np.int32, (what, "B")
    assert lat.score.tobytes() == tabs["score"].tobytes(), (what, "score")
    assert np.array_equal(lat.final_word, tabs["final"]), (what, "final")


def _assert_backward(back, path, tabs, what):
    for f in BACK:
        got = getattr(back, f)
        assert got.dtype == tabs[f].dtype and np.array_equal(got, tabs[f]), (what, f)
    assert path.score.tobytes() == tabs["root"].tobytes(), (what, "root")
    for f in ("n_words", "path_word", "path_entry"):
        assert np.array_equal(getattr(path, f), tabs[f]), (what, f)


@pytest.mark.parametrize("exits", lc.EXITS)
@pytest.mark.parametrize("topology", lc.TOPOLOGIES)
@pytest.mark.parametrize("W,S", lc.SHAPES)
def test_tables_equal_the_definition(W, S, topology, exits):
    """Random ``logb``; ``lm`` dense random with about a third of the pairs forbidden and one unreachable word; the
    backward pass and the walk under ``lm`` and under a second random ``lm'``."""
    from sapr_amd.connected import WordBigram, connected_viterbi
    what = (W, S, topology, exits)
    ls, lt, lx, lm, lm2, logb, dead = lc.random_case(W, S, topology, exits)
    per, tabs, per2, tabs2 = lc.reference(W, S, topology, exits)
    net = _net(ls, lt, lx, lm)
    lat = connected_lattice(logb, LENGTHS, net)
    _assert_forward(lat, tabs, what)
    _assert_backward(lat.backward(), lat.best(), tabs, what)
    other = WordBigram(*lm2)
    _assert_backward(lat.backward(other), lat.rescore(other), tabs2, (what, "lm'"))
    assert lat.backward() is lat.backward()                      # the network's own result is kept
    # the one-pass search on the same network: its score bit for bit, and (the best string is unique) its path
    res = connected_viterbi(logb, LENGTHS, net)
    assert lat.score.tobytes() == res.score.tobytes()
    best = lat.best()
    assert np.array_equal(best.path_word, res.path_word) and np.array_equal(best.path_entry, res.path_entry)
    assert np.array_equal(best.n_words, res.n_words)
    assert [best.segments(u) for u in range(len(LENGTHS))] == [res.segments(u) for u in range(len(LENGTHS))]
    # the empty utterance scores -inf and has no records; the dead word has no record on a complete path
    e = LENGTHS.index(0)
    assert lat.score[e] == NEG and best.score[e] == NEG and lat.records(e) == [] and best.n_words[e] == 0
    margin = lat.margins()
    assert np.array_equal(margin, np.concatenate([p["margin"] for p in per]))
    if W > 1:
        assert (margin[:, dead] == NEG).all() and not lat.prune(np.inf)[:, dead].any()
    assert np.allclose(lat.eps(), [p["eps"] for p in per], rtol=1e-12, atol=0)
    for beam in (0.0, 3.0, np.inf):
        want = np.concatenate([lref.kept(p["margin"], beam, p["eps"]) for p in per])
        assert np.array_equal(lat.prune(beam), want), (what, beam)
    u = 3                                                         # 65 frames
    assert [(w, a, b) for w, a, b, _, _ in lat.records(u, 0.0)] == res.segments(u)


def test_network_without_a_bigram_runs_under_its_word_penalty():
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    W, S = 11, 10
    ls, lt, lx, _, _, logb, _ = lc.random_case(W, S, "dense", "any")
    for p in (0.0, -7.25):
        net = ConnectedNetwork(ls, lt, lx, word_penalty=p)
        lat = connected_lattice(logb, LENGTHS, net)
        res = connected_viterbi(logb, LENGTHS, net)
        assert lat.score.tobytes() == res.score.tobytes(), p
        _, tabs = lref.batch(logb, LENGTHS, ls, lt, lx, *bref.word_loop_lm(W, p))
        _assert_forward(lat, tabs, p)
        _assert_backward(lat.backward(), lat.best(), tabs, p)


def test_exact_ties_go_to_the_lowest_index():
    logb, ls, lt, lx, lm, lm0, lm1, expected = bref.tie_case()
    lat = connected_lattice(np.concatenate([logb, logb]), [4, 4], _net(ls, lt, lx, (lm, lm0, lm1)))
    _, tabs = lref.batch(np.concatenate([logb, logb]), [4, 4], ls, lt, lx, lm, lm0, lm1)
    _assert_forward(lat, tabs, "ties")
    _assert_backward(lat.backward(), lat.best(), tabs, "ties")
    best = lat.best()
    assert lat.tables()[2][:4].tolist() == [[0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1]]
    assert best.score.tolist() == [expected[0]] * 2 and best.n_words.tolist() == [expected[1]] * 2
    assert best.path_word.tolist() == expected[2].tolist() * 2
    assert best.path_entry.tolist() == expected[4].tolist() * 2
    assert lat.backward().first.tolist() == [[0, 0], [0, 0]]


def _bytes(lat, bigram=None):
    back = lat.backward(bigram)
    path = lat.rescore(bigram)
    return [a.tobytes() for a in lat.tables()] + [lat.score.tobytes(), lat.final_word.tobytes()] + \
        [getattr(back, f).tobytes() for f in BACK] + [path.n_words.tobytes(), path.path_word.tobytes(),
                                                      path.path_entry.tobytes()]


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import WordBigram
    W, S = 11, 10
    ls, lt, lx, lm, lm2, logb, _ = lc.random_case(W, S, "dense", "any")
    net, other = _net(ls, lt, lx, lm), WordBigram(*lm2)
    offs = np.r_[0, np.cumsum(LENGTHS)]
    a, b = connected_lattice(logb, LENGTHS, net), connected_lattice(logb, LENGTHS, net)
    assert _bytes(a) == _bytes(b) and _bytes(a, other) == _bytes(b, other)
    rows = ("X", "N", "B", "beta", "next_end", "next_word", "path_word", "path_entry")
    for u in (1, 3, 8):
        lo, hi = offs[u], offs[u + 1]
        one = connected_lattice(logb[lo:hi], [LENGTHS[u]], net)
        for bg in (None, other):
            back, path, wb, wp = one.backward(bg), one.rescore(bg), a.backward(bg), a.rescore(bg)
            got = dict(zip(rows, one.tables() + (back.beta, back.next_end, back.next_word, path.path_word,
                                                 path.path_entry)))
            want = dict(zip(rows, a.tables() + (wb.beta, wb.next_end, wb.next_word, wp.path_word, wp.path_entry)))
            for f in rows:
                assert got[f].tobytes() == want[f][lo:hi].tobytes(), (u, f)
            assert back.root.tobytes() == wb.root[u:u + 1].tobytes() and np.array_equal(back.first[0], wb.first[u])
            assert path.n_words[0] == wp.n_words[u] and one.score.tobytes() == a.score[u:u + 1].tobytes()
    # a NaN frame in utterance 3 (65 frames): every other utterance keeps its bytes, and the walk stays in range
    bad = logb.copy()
    bad[offs[3] + 20] = np.nan
    c = connected_lattice(bad, LENGTHS, net)
    keep = np.ones(len(logb), bool)
    keep[offs[3]:offs[4]] = False
    others = np.arange(len(LENGTHS)) != 3
    for bg in (None, other):
        cb, cp, ab, ap = c.backward(bg), c.rescore(bg), a.backward(bg), a.rescore(bg)
        for x, y in zip(c.tables() + (cb.beta, cb.next_end, cb.next_word, cp.path_word, cp.path_entry),
                        a.tables() + (ab.beta, ab.next_end, ab.next_word, ap.path_word, ap.path_entry)):
            assert x[keep].tobytes() == y[keep].tobytes()
        assert cb.root[others].tobytes() == ab.root[others].tobytes()
        assert np.array_equal(cb.first[others], ab.first[others])
        assert np.array_equal(cp.n_words[others], ap.n_words[others])
        pw = cp.path_word[offs[3]:offs[4]]
        assert pw.min() >= -1 and pw.max() <= W - 1 and 0 <= cp.n_words[3] <= LENGTHS[3]
        assert cb.next_end[offs[3]:offs[4]].max() <= LENGTHS[3] - 1
    assert c.score[others].tobytes() == a.score[others].tobytes()
    for u in range(len(LENGTHS)):
        for w, s, e, _, _ in c.records(u):
            assert 0 <= w < W and 0 <= s < e <= LENGTHS[u]


# ---- end to end: Decoder.decode_connected(lattice=beam) over the three emission families ----------------------------
@pytest.mark.parametrize("family,impl", [("diag", "hmmlearn"), ("full", "hmmlearn"), ("gmm", "gmmhmm")])
def test_decoder_lattice_rescored_under_the_grammar(tmp_path, family, impl):
    """``_bigram_ref``'s committed case (words 2 and 3 share their Gaussians): decode under the free loop with a
    lattice, rescore the lattice under the grammar, compare with ``decode_connected(bigram=grammar)``.  The rescored
    score is never above the re-decode by more than eps_u; on the utterances where tests/test_lattice_cpu.py found the
    two equal from the definition alone the strings match, and one of them differs from the free loop's."""
    from sapr_amd import connected
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    from sapr_amd.decoder import Decoder
    from tests.test_bigram_gpu import _models, _pickle_models
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, truth, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(),
                                                    shared=bref.E2E_SHARED)
    names = list(lc.E2E_NAMES)
    root = _pickle_models(tmp_path, impl, _models(family, model), names)
    dec = Decoder(models_dir=root, implementation=impl, n_iter=15)
    pos = {c: dec.vocab.index(names[c]) for c in range(W)}       # load order (glob) is the word order of the network
    grammar = WordBigram.from_grammar(W, [(pos[a], pos[b]) for a, b in bref.E2E_PAIRS],
                                      starts=[pos[a] for a in bref.E2E_STARTS])
    feats = [x.T for x in utts]
    beam = 25.0
    plain = dec.decode_connected(feats)
    free = dec.decode_connected(feats, lattice=beam)
    regram = dec.decode_connected(feats, bigram=grammar)
    for a, b in zip(plain, free):                                # every other key is as it is without the argument
        assert set(b) == set(a) | {"lattice"}
        assert all(np.array_equal(a[k], b[k]) for k in a)
    net = ConnectedNetwork.from_models([dec.models[w] for w in dec.vocab], names=dec.vocab, implementation=impl)
    assert net.family == family
    lat = connected.connected_decode(utts, net, lattice=True).lattice
    assert lat.score.tolist() == [row["log_likelihood"] for row in free]
    path, eps = lat.rescore(grammar), lat.eps()
    order = tuple(names.index(w) for w in dec.vocab)             # (tests/test_lattice_cpu.py: 2 before 3 and 3 before 2)
    rows = lc.e2e(order)
    reached = differ = wider = 0
    for u, row in enumerate(free):
        assert row["lattice"] == [(dec.vocab[w], a, b, ac, m) for w, a, b, ac, m in lat.records(u, beam)]
        kept = [(w, a, b) for w, a, b, _, _ in row["lattice"]]
        assert all(seg in kept for seg in row["segments"])
        wider += len(kept) > len(row["segments"])
        assert all(-(beam + eps[u]) <= m <= eps[u] for *_, m in row["lattice"])
        assert path.score[u] <= regram[u]["log_likelihood"] + eps[u]
        assert [dec.vocab[w] for w in rows[u]["free_words"]] == row["words"]   # the CPU case is this case
        if rows[u]["reach"]:
            reached += 1
            assert [dec.vocab[w] for w in path.words(u)] == regram[u]["words"], u
            assert [(dec.vocab[w], a, b) for w, a, b in path.segments(u)] == regram[u]["segments"], u
            differ += regram[u]["words"] != row["words"]
    assert reached >= 1 and differ >= 1 and wider >= 1
    share = np.mean([abs(path.score[u] - regram[u]["log_likelihood"]) <= eps[u] for u in range(n)])
    print(f"lattice rescoring reaches the re-decode on {share:.0%} of {n} utterances ({family})")
    # lattice=True: every record on a complete path
    full = dec.decode_connected(feats[:2], lattice=True)
    assert [len(r["lattice"]) for r in full] == [len(lat.records(u, np.inf)) for u in range(2)]
