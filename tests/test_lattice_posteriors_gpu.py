"""GPU: lattice posteriors (the three kernels behind ``sapr_connected_lattice_posteriors`` in
csrc/connected_lattice.hip) through ``WordLattice.posteriors`` against the CPU restatement
tests/_lattice_post_ref.py, which is the definition.  The tolerances are the pins of tests/test_loop_posteriors_gpu.py:
rtol 1e-11 on a finite log-likelihood (non-finite values must be equal), rtol = atol = 1e-9 on the posterior tables.
tests/test_lattice_posteriors_cpu.py checks the definition itself against the enumeration of every lattice path."""
import functools

import numpy as np
import pytest

from sapr_amd.connected import connected_lattice
from tests import _bigram_ref as bref
from tests import _lattice_cases as lc
from tests import _lattice_post_ref as pref

pytestmark = pytest.mark.gpu

NEG = -np.inf
LENGTHS = lc.LENGTHS
OFFS = np.r_[0, np.cumsum(LENGTHS)]
LL_RTOL, POST_TOL = 1e-11, 1e-9
KAPPAS = (1.0, 0.125)


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


@functools.lru_cache(maxsize=None)
def _want(W, S, topology, exits, other, kappa):
    """The definition on the case's reference tables, computed once; nobody writes to it."""
    _, _, _, lm, lm2, _, _ = lc.random_case(W, S, topology, exits)
    _, tabs, _, _ = lc.reference(W, S, topology, exits)
    return pref.batch(tabs, LENGTHS, lm[1], *(lm2 if other else lm), kappa=kappa)[1]


def _assert_close(got, want, what):
    fin = np.isfinite(want["loglik"])
    assert np.array_equal(got.loglik[~fin], want["loglik"][~fin], equal_nan=True), (what, "loglik")
    assert np.allclose(got.loglik[fin], want["loglik"][fin], rtol=LL_RTOL, atol=0), (what, "loglik")
    for f in ("record_post", "word_post"):
        g, w = getattr(got, f), want[f]
        assert g.shape == w.shape and g.dtype == np.float64
        print(what, f, "max deviation", float(np.abs(g - w).max()) if w.size else 0.0)
        assert np.allclose(g, w, rtol=POST_TOL, atol=POST_TOL), (what, f, float(np.abs(g - w).max()))


@pytest.mark.parametrize("exits", lc.EXITS)
@pytest.mark.parametrize("topology", lc.TOPOLOGIES)
@pytest.mark.parametrize("W,S", lc.SHAPES)
def test_posteriors_equal_the_definition(W, S, topology, exits):
    """Every lattice case, at kappa = 1 and 1/8, under the lattice's own tables and under ``lm2``; the rows of
    ``word_post`` sum to 1 wherever ``loglik`` is finite, the dead word's columns are exact zeros under ``lm`` and the
    empty utterance has ``loglik`` -inf."""
    from sapr_amd.connected import WordBigram
    ls, lt, lx, lm, lm2, logb, dead = lc.random_case(W, S, topology, exits)
    lat = connected_lattice(logb, LENGTHS, _net(ls, lt, lx, lm))
    finite = 0
    for other in (False, True):
        for kappa in KAPPAS:
            what = (W, S, topology, exits, "lm2" if other else "lm", kappa)
            got = lat.posteriors(WordBigram(*lm2) if other else None, acoustic_scale=kappa)
            _assert_close(got, _want(W, S, topology, exits, other, kappa), what)
            assert np.array_equal(got.offsets, OFFS)
            rows = np.repeat(np.isfinite(got.loglik), LENGTHS)
            assert np.allclose(got.word_post[rows].sum(axis=1), 1.0, rtol=0, atol=POST_TOL), what
            assert not got.word_post[~rows].any() and not got.record_post[~rows].any(), what
            assert got.loglik[LENGTHS.index(0)] == NEG
            if W > 1 and not other:
                assert not got.word_post[:, dead].any() and not got.record_post[:, dead].any(), what
            finite += int(np.isfinite(got.loglik).sum())
    assert finite >= 20


def test_scaled_posteriors_are_not_zeros_and_ones():
    """At kappa = 1 most records' posteriors are 0 or 1 to six digits; at kappa = 1/8 at least 90 % of the records
    that carry mass lie strictly inside (1e-6, 1 - 1e-6), so the parity above does not compare zeros with ones."""
    inside = {k: 0 for k in KAPPAS}
    mass = {k: 0 for k in KAPPAS}
    for W, S in ((3, 4), (11, 10), (14, 18), (64, 4)):
        ls, lt, lx, lm, _, logb, _ = lc.random_case(W, S, "dense", "any")
        lat = connected_lattice(logb, LENGTHS, _net(ls, lt, lx, lm))
        for kappa in KAPPAS:
            rp = lat.posteriors(acoustic_scale=kappa).record_post
            mass[kappa] += int((rp > 0).sum())
            inside[kappa] += int(((rp > 1e-6) & (rp < 1 - 1e-6)).sum())
    print("records with mass", mass, "strictly inside", inside)
    assert mass[0.125] >= 10000 and inside[0.125] >= 0.9 * mass[0.125]


@pytest.mark.parametrize("W,S", lc.SHAPES)
def test_beams(W, S):
    """``beam=0`` at kappa = 1 leaves the best path alone: its records have posterior 1, ``word_post`` is the one-hot
    of the best string and ``loglik`` its score within eps_u.  ``beam=inf`` drops only records on no complete path:
    it equals ``beam=None``."""
    ls, lt, lx, lm, _, logb, _ = lc.random_case(W, S, "dense", "any")
    lat = connected_lattice(logb, LENGTHS, _net(ls, lt, lx, lm))
    best, eps = lat.best(), lat.eps()
    for kappa in KAPPAS:
        every, wide = lat.posteriors(acoustic_scale=kappa), lat.posteriors(acoustic_scale=kappa, beam=np.inf)
        fin = np.isfinite(every.loglik)
        assert np.array_equal(np.isfinite(wide.loglik), fin) and np.array_equal(wide.loglik[~fin], every.loglik[~fin])
        assert np.allclose(wide.loglik[fin], every.loglik[fin], rtol=LL_RTOL, atol=0)
        on = every.record_post > 0
        assert np.allclose(wide.record_post[on], every.record_post[on], rtol=0, atol=POST_TOL)
        assert np.allclose(wide.word_post, every.word_post, rtol=0, atol=POST_TOL)
    one = lat.posteriors(beam=0.0)
    want_rec = np.zeros_like(one.record_post)
    want_word = np.zeros_like(one.word_post)
    paths = 0
    for u in range(len(LENGTHS)):
        for w, a, b, _, _ in lat.records(u, 0.0):
            want_rec[OFFS[u] + b - 1, w] = 1.0
        if best.n_words[u]:
            paths += 1
            want_word[np.arange(OFFS[u], OFFS[u + 1]), best.path_word[OFFS[u]:OFFS[u + 1]]] = 1.0
            assert abs(one.loglik[u] - lat.score[u]) <= eps[u], (u, one.loglik[u], lat.score[u], eps[u])
        else:
            assert one.loglik[u] == NEG
    assert paths >= 5 and want_rec.sum() == best.n_words.sum()
    assert np.allclose(one.record_post, want_rec, rtol=0, atol=POST_TOL)
    assert np.allclose(one.word_post, want_word, rtol=0, atol=POST_TOL)


def test_every_pair_forbidden_leaves_one_word_per_utterance():
    """Under a grammar without pairs (open starts and ends) an utterance is one word: ``loglik`` is
    lse_w kappa X_{T-1}(w) and every row of ``word_post`` the softmax of those."""
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    W, S = 11, 10
    ls, lt, lx, _, _, logb, _ = lc.random_case(W, S, "dense", "any")
    grammar = WordBigram.from_grammar(W, [])
    lat = connected_lattice(logb, LENGTHS, ConnectedNetwork(ls, lt, lx, bigram=grammar))
    X = lat.tables()[0]
    for kappa in KAPPAS:
        for got in (lat.posteriors(acoustic_scale=kappa), lat.posteriors(grammar, acoustic_scale=kappa)):
            finite = 0
            for u, T in enumerate(LENGTHS):
                rows = got.word_post[OFFS[u]:OFFS[u + 1]]
                last = kappa * X[OFFS[u + 1] - 1] if T else np.full(W, NEG)
                ll = float(pref.lse(last))
                if not np.isfinite(ll):
                    assert got.loglik[u] == NEG and not rows.any()
                    continue
                finite += 1
                assert np.isclose(got.loglik[u], ll, rtol=LL_RTOL, atol=0), u
                assert np.allclose(rows, np.exp(last - ll)[None, :], rtol=POST_TOL, atol=POST_TOL), u
            assert finite >= 5


def _bytes(post):
    return [post.loglik.tobytes(), post.record_post.tobytes(), post.word_post.tobytes()]


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import WordBigram
    W, S = 11, 10
    ls, lt, lx, lm, lm2, logb, _ = lc.random_case(W, S, "dense", "any")
    net, other = _net(ls, lt, lx, lm), WordBigram(*lm2)
    a = connected_lattice(logb, LENGTHS, net)
    kw = dict(acoustic_scale=0.125, beam=40.0)
    assert _bytes(a.posteriors(other, **kw)) == _bytes(a.posteriors(other, **kw))
    assert _bytes(a.posteriors()) == _bytes(connected_lattice(logb, LENGTHS, net).posteriors())
    whole = a.posteriors(other, acoustic_scale=0.125)
    for u in (1, 3, 8):                      # an utterance on its own returns the rows it has in the batch
        lo, hi = OFFS[u], OFFS[u + 1]
        one = connected_lattice(logb[lo:hi], [LENGTHS[u]], net).posteriors(other, acoustic_scale=0.125)
        assert one.loglik.tobytes() == whole.loglik[u:u + 1].tobytes()
        assert one.record_post.tobytes() == whole.record_post[lo:hi].tobytes()
        assert one.word_post.tobytes() == whole.word_post[lo:hi].tobytes()
    # a NaN frame in utterance 3 (65 frames): every other utterance keeps its bytes
    bad = logb.copy()
    bad[OFFS[3] + 20] = np.nan
    c = connected_lattice(bad, LENGTHS, net).posteriors(other, acoustic_scale=0.125)
    keep = np.ones(len(logb), bool)
    keep[OFFS[3]:OFFS[4]] = False
    others = np.arange(len(LENGTHS)) != 3
    assert c.loglik[others].tobytes() == whole.loglik[others].tobytes()
    assert c.record_post[keep].tobytes() == whole.record_post[keep].tobytes()
    assert c.word_post[keep].tobytes() == whole.word_post[keep].tobytes()


# ---- end to end: Decoder.decode_connected(confidence="lattice") over the three emission families -------------------
@pytest.mark.parametrize("family,impl", [("diag", "hmmlearn"), ("full", "hmmlearn"), ("gmm", "gmmhmm")])
def test_decoder_lattice_confidence(tmp_path, family, impl):
    """``_bigram_ref``'s committed case (words 2 and 3 share their Gaussians).  Under the free loop the lattice cannot
    tell the two apart: their segments have confidence 0.5 and a slot that lists both, every other segment more than
    0.99; under the grammar every segment has more than 0.99."""
    from sapr_amd.connected import WordBigram
    from sapr_amd.decoder import Decoder
    from tests.test_bigram_gpu import _models, _pickle_models
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, _, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(), shared=bref.E2E_SHARED)
    names = list(lc.E2E_NAMES)
    root = _pickle_models(tmp_path, impl, _models(family, model), names)
    dec = Decoder(models_dir=root, implementation=impl, n_iter=15)
    pos = {c: dec.vocab.index(names[c]) for c in range(W)}
    grammar = WordBigram.from_grammar(W, [(pos[a], pos[b]) for a, b in bref.E2E_PAIRS],
                                      starts=[pos[a] for a in bref.E2E_STARTS])
    feats = [x.T for x in utts]
    twins = {names[2], names[3]}
    plain = dec.decode_connected(feats)
    free = dec.decode_connected(feats, confidence="lattice")
    halves = 0
    for a, b in zip(plain, free):
        assert set(b) == set(a) | {"confidence", "lattice_log_likelihood", "slots"}
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert len(b["confidence"]) == len(b["slots"]) == len(b["segments"])
        assert b["lattice_log_likelihood"] >= b["log_likelihood"] - 1e-9 * abs(b["log_likelihood"])
        for (word, _, _), conf, slot in zip(b["segments"], b["confidence"], b["slots"]):
            assert abs(sum(p for _, p in slot) - 1.0) <= POST_TOL and dict(slot)[word] == conf
            if word in twins:
                halves += 1
                assert abs(conf - 0.5) <= POST_TOL, (word, conf)
                assert {w for w, _ in slot[:2]} == twins        # (both, ahead of whatever else carries mass)
            else:
                assert conf > 0.99, (word, conf)
    assert halves >= 3
    for row in dec.decode_connected(feats, bigram=grammar, confidence="lattice"):
        assert row["confidence"] and all(c > 0.99 for c in row["confidence"]), row["confidence"]
    # lattice= beside it: one lattice recursion serves both, and each key is what it is alone
    both = dec.decode_connected(feats[:3], confidence="lattice", lattice=25.0, acoustic_scale=0.125)
    alone = dec.decode_connected(feats[:3], lattice=25.0)
    scaled = dec.decode_connected(feats[:3], confidence="lattice", acoustic_scale=0.125)
    for a, b, c in zip(both, alone, scaled):
        assert a["lattice"] == b["lattice"] and a["confidence"] == c["confidence"] and a["slots"] == c["slots"]
    # confidence=True is the word loop's forward-backward, as before
    loop = dec.decode_connected(feats[:3], confidence=True)
    for a, b in zip(plain, loop):
        assert set(b) == set(a) | {"confidence", "total_log_likelihood", "log_posterior"}
