"""GPU: forced alignment (csrc/connected_align.hip) through the C ABI and the Python layer against the CPU restatement
tests/_align_ref.py.  Every comparison with the restatement's recursion is ``np.array_equal``: no tolerance.
tests/test_align_cpu.py checks that the recursion cases have paths and that the consistency cases have no exact ties."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _connected_ref as ref

pytestmark = pytest.mark.gpu

NEG = -np.inf
FIELDS = ("score", "path_word", "path_state", "path_entry", "word_start")


def _assert_equal(res, want, what):
    for f, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, f), w), (f, what)     # (bit-equal: -inf == -inf, no NaN in these cases)


def _raw_align(logb, lengths, transcripts, ls, lt, lx, pen, max_words):
    """``sapr_connected_align`` itself, with transcripts the Python layer refuses (too long for ``max_words``, indices
    outside the vocabulary): ``(score, path_word, path_state, path_entry, word_start)`` on the host."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.connected import layout
    W, S = ls.shape
    SP = layout(W, S)[0]
    total = int(sum(lengths))
    wide = np.full((total, W, SP), NEG)
    wide[:, :, :S] = logb
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])].astype(np.int64)
    words = np.concatenate([np.asarray(t, np.int32) for t in transcripts]).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.sapr_connected_align_workspace_bytes(total, len(lengths), max_words, S, C.byref(n)) == 0
    guard = 4096                                                 # the bytes behind the workspace must stay untouched
    ws = torch.full((n.value + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    t_logb, t_offs, t_woffs, t_words, t_ls, t_lt, t_lx = (dev(a) for a in (wide, offs, woffs, words, ls, lt, lx))
    score = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")
    start = torch.empty(len(words), dtype=torch.int32, device="cuda")
    _lib.check(lib.sapr_connected_align(
        _lib.ptr(t_logb), _lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words), _lib.ptr(t_woffs), len(words),
        max_words, _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx), pen, W, S, _lib.ptr(ws), n.value, _lib.ptr(score),
        _lib.ptr(pw), _lib.ptr(ps), _lib.ptr(pe), _lib.ptr(start), _lib.current_stream()), "sapr_connected_align")
    torch.cuda.synchronize()
    assert bool((ws[n.value:] == 0xA5).all())
    return tuple(a.cpu().numpy() for a in (score, pw, ps, pe, start))


@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_recursion_equals_reference(W, S, max_words, topology, exits):
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    lengths = aref.RECURSION_LENGTHS
    for integer in (False, True):
        ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, topology, exits, integer)
        assert max(len(t) for t in transcripts) == max_words or max_words == 64
        for pen in aref.PENALTIES:
            res = align_viterbi(logb, lengths, transcripts, ConnectedNetwork(ls, lt, lx, word_penalty=pen))
            want = aref.align_batch(logb, lengths, transcripts, ls, lt, lx, pen)
            _assert_equal(res, want, (integer, pen))
            assert int(np.isfinite(res.score).sum()) >= 6
            for u in (lengths.index(0), lengths.index(1), lengths.index(2)):
                assert res.score[u] == NEG and res.segments(u) == []
            for u in np.flatnonzero(np.isfinite(res.score)):
                segs = res.segments(u)
                assert [w for w, _, _ in segs] == transcripts[u] and segs[0][1] == 0 and segs[-1][2] == lengths[u]


def test_pathless_transcripts_at_the_c_abi():
    """What the Python layer refuses earlier: a transcript longer than the ``max_words`` the call was sized for and
    word indices outside 0 .. W - 1 make their own utterance pathless, and nothing else changes."""
    W, S, max_words = 5, 7, 4
    ls, lt, lx, logb, _ = aref.recursion_case(W, S, 25, "skip", "any", False)
    lengths = [40, 64, 30, 3, 50]
    logb = logb[:sum(lengths)]
    good = [[1, 4, 4], [0, 2, 3, 1], [2], [3], [4, 0]]
    bad = [[1, 4, 4], [0, 2, 3, 1, 0], [W], [-1], [4, 0]]
    want = aref.align_batch(logb, lengths, good, ls, lt, lx, -1.5)
    assert np.isfinite(want[0]).all()
    offs = np.r_[0, np.cumsum(lengths)]
    woffs = np.r_[0, np.cumsum([len(t) for t in bad])]
    gwoffs = np.r_[0, np.cumsum([len(t) for t in good])]
    got = _raw_align(logb, lengths, bad, ls, lt, lx, -1.5, max_words)
    for u in (0, 4):
        assert got[0][u] == want[0][u]
        for k in (1, 2, 3):
            assert np.array_equal(got[k][offs[u]:offs[u + 1]], want[k][offs[u]:offs[u + 1]])
        assert np.array_equal(got[4][woffs[u]:woffs[u + 1]], want[4][gwoffs[u]:gwoffs[u + 1]])
    for u in (1, 2, 3):
        assert got[0][u] == NEG
        assert (got[1][offs[u]:offs[u + 1]] == -1).all() and (got[2][offs[u]:offs[u + 1]] == -1).all()
        assert not got[3][offs[u]:offs[u + 1]].any() and (got[4][woffs[u]:woffs[u + 1]] == -1).all()
    # sized for the transcripts it gets, the same entry point answers as the restatement does
    for a, b in zip(_raw_align(logb, lengths, good, ls, lt, lx, -1.5, max_words), want):
        assert np.array_equal(a, b)


def test_one_word_equals_the_word_loop_over_that_word():
    """K = 1: the chain is one word model, and so is the word loop over the one-word network cut from the vocabulary
    once re-entering is priced at -inf."""
    from sapr_amd.connected import ConnectedNetwork, align_viterbi, connected_viterbi
    rng = np.random.default_rng(21)
    W, S = 11, 10
    ls, lt, lx = aref.network(rng, W, S, "bidiag", "last", False)
    lengths = [12, 64, 10, 5, 130]                               # (5 frames do not reach the last of 10 states)
    logb = rng.normal(-40.0, 15.0, (sum(lengths), W, S))
    for w in (0, 6, 10):
        res = align_viterbi(logb, lengths, [[w]] * len(lengths), ConnectedNetwork(ls, lt, lx, word_penalty=-3.0))
        one = connected_viterbi(logb[:, w:w + 1], lengths,
                                ConnectedNetwork(ls[w:w + 1], lt[w:w + 1], lx[w:w + 1], word_penalty=NEG))
        assert np.array_equal(res.score, one.score) and np.isfinite(res.score).sum() == 4
        assert np.array_equal(res.path_state, one.path_state) and np.array_equal(res.path_entry, one.path_entry)
        assert np.array_equal(res.path_word, np.where(one.path_word < 0, -1, w))


def test_alignment_is_deterministic_and_independent_of_the_batch():
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    W, S, max_words = 11, 18, 5
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "dense", "any", False)
    lengths = aref.RECURSION_LENGTHS
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-2.0)
    a, b = (align_viterbi(logb, lengths, transcripts, net) for _ in range(2))
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (1, 3, 9):
        lo, hi = a.offsets[u], a.offsets[u + 1]
        one = align_viterbi(logb[lo:hi], [lengths[u]], [transcripts[u]], net)
        assert one.score.tobytes() == a.score[u:u + 1].tobytes()
        for f in ("path_word", "path_state", "path_entry"):
            assert np.array_equal(getattr(one, f), getattr(a, f)[lo:hi]), f
        assert np.array_equal(one.word_start, a.word_start[a.word_offsets[u]:a.word_offsets[u + 1]])


def test_alignment_ignores_the_padded_columns_of_logb():
    """(5, 7) runs in SP = 10: whatever finite value the caller leaves in the three padded columns changes nothing."""
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    W, S, SP = 5, 7, 10
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, 25, "skip", "last", False)
    lengths = aref.RECURSION_LENGTHS
    wide = np.random.default_rng(3).normal(50.0, 5.0, (sum(lengths), W, SP))
    wide[:, :, :S] = logb
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-1.5)
    want = aref.align_batch(logb, lengths, transcripts, ls, lt, lx, -1.5)
    assert np.isfinite(want[0]).sum() >= 6
    _assert_equal(align_viterbi(wide, lengths, transcripts, net), want, "wide")
    _assert_equal(align_viterbi(wide.reshape(-1, W * SP), lengths, transcripts, net), want, "flat")


def test_a_nan_frame_stays_inside_its_utterance():
    W, S, max_words = 14, 18, 14
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "dense", "any", False)
    lengths = aref.RECURSION_LENGTHS
    offs = np.r_[0, np.cumsum(lengths)]
    clean = _raw_align(logb, lengths, transcripts, ls, lt, lx, -2.0, max_words)
    hit = lengths.index(300)
    assert np.isfinite(clean[0][hit])
    dirty = logb.copy()
    dirty[offs[hit] + 150] = np.nan
    got = _raw_align(dirty, lengths, transcripts, ls, lt, lx, -2.0, max_words)   # (the guard checks the workspace)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])]
    for u in range(len(lengths)):
        if u == hit:
            continue
        assert got[0][u:u + 1].tobytes() == clean[0][u:u + 1].tobytes()
        for k in (1, 2, 3):
            assert np.array_equal(got[k][offs[u]:offs[u + 1]], clean[k][offs[u]:offs[u + 1]])
        assert np.array_equal(got[4][woffs[u]:woffs[u + 1]], clean[4][woffs[u]:woffs[u + 1]])
    lo, hi = offs[hit], offs[hit + 1]
    assert not np.isfinite(got[0][hit])                          # nothing is repaired: the utterance has no path
    assert (got[1][lo:hi] == -1).all() and (got[2][lo:hi] == -1).all() and not got[3][lo:hi].any()
    assert (got[4][woffs[hit]:woffs[hit + 1]] == -1).all()


# ---- consistency with the word loop, all three families ---------------------------------------------------------
def _diag_network(model, pen):
    from sapr_amd.connected import ConnectedNetwork
    return ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], pen, None, model["means"],
                            model["vars"], model["gconst"])


def _family_case(family, spec, pen):
    """``(network, utterances, truth)`` of a committed case of any family."""
    from sapr_amd.connected import ConnectedNetwork
    if family == "diag":
        model, utts, truth = ref.sample_case(*spec)
        return _diag_network(model, pen), utts, truth
    model, utts, truth = cases.case(family, spec)
    return ConnectedNetwork.from_models(cases.models_of(family, model), word_penalty=pen), utts, truth


CONSISTENCY = ([("diag", c) for c in ref.E2E_CASES] + [("gmm", c) for c in cases.GMM_CASES]
               + [("full", c) for c in cases.FULL_CASES])


@pytest.mark.parametrize("family,spec", CONSISTENCY)
def test_aligning_to_the_decoded_string_reproduces_the_word_loop(family, spec):
    """``connected_decode``, then ``connected_align`` with the decoded strings, on the same emitted bits: scores ``==``
    and equal path rows.  Aligned to the sampled truth instead, the score is finite and no greater than the free one."""
    from sapr_amd.connected import connected_align, connected_decode
    for pen in (0.0, -7.5):
        net, utts, truth = _family_case(family, spec, pen)
        free = connected_decode(utts, net)
        assert np.isfinite(free.score).all()
        decoded = [free.words(u) for u in range(len(utts))]
        res = connected_align(utts, decoded, net)
        assert np.array_equal(res.score, free.score)
        for f in ("path_word", "path_state", "path_entry"):
            assert np.array_equal(getattr(res, f), getattr(free, f)), f
        assert np.array_equal(res.word_start, np.concatenate(
            [np.flatnonzero(free.path_entry[a:b]) for a, b in zip(free.offsets[:-1], free.offsets[1:])]))
        for u in range(len(utts)):
            assert res.segments(u) == free.segments(u)
        forced = connected_align(utts, truth, net)
        assert np.isfinite(forced.score).all() and (forced.score <= free.score).all()
        same = [u for u in range(len(utts)) if decoded[u] == truth[u]]
        assert np.array_equal(forced.score[same], free.score[same]) and len(same) >= len(utts) // 2


# ---- Decoder.align ---------------------------------------------------------------------------------------------
def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def _diag_decoder_case():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    seed, W, S, D, n = ref.DECODER_CASE
    model, utts, truth = ref.sample_case(seed, W, S, D, n, spherical=True)
    models = []
    for w in range(W):
        m = GaussianHMM(n_components=S, covariance_type="spherical" if w % 2 else "diag")
        m.startprob_, m.transmat_, m.means_ = model["startprob"][w], model["transmat"][w], model["means"][w]
        m._covars_ = model["vars"][w, :, 0].copy() if w % 2 else model["vars"][w]
        models.append(m)
    logb = np.concatenate([ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts])
    return model, utts, truth, models, logb


@pytest.mark.parametrize("family,impl,rtol", [("diag", "hmmlearn", 1e-12), ("gmm", "gmmhmm", 1e-11),
                                              ("full", "hmmlearn", 1e-11)])
def test_decoder_align(tmp_path, family, impl, rtol):
    """Word names in and out over pickled models — diag + spherical, ``GMMHMM``, diag + spherical + tied + full —
    against the restatement on the family's reference emission: equal paths and boundaries; the score within the
    family's bound on its log scores (1e-12 relative for diag, 1e-11 for the mixtures and the full covariances, the
    pins of tests/test_connected_gpu.py and tests/test_connected_families_gpu.py: a score is a sum of negative terms)."""
    from sapr_amd.decoder import Decoder
    names = ["zero", "one", "two", "three"]
    if family == "diag":
        model, utts, truth, models, logb = _diag_decoder_case()
    else:
        spec = cases.GMM_DECODER_CASE if family == "gmm" else cases.FULL_DECODER_CASE
        model, utts, truth = cases.case(family, spec)
        models = cases.models_of(family, model)
        logb = cases.case_logb(family, spec)[0]
    dec = Decoder(models_dir=_pickle_models(tmp_path, impl, models, names), implementation=impl, n_iter=15)
    order = [names.index(w) for w in dec.vocab]                  # load order (glob) is the word order of the network
    rank = {w: k for k, w in enumerate(order)}
    lengths = [len(x) for x in utts]
    offs = np.r_[0, np.cumsum(lengths)]
    said = [[names[w] for w in words] for words in truth]
    indices = [[rank[w] for w in words] for words in truth]
    W, S = model["log_start"].shape
    worst = 0.0
    for pen in (0.0, -30.0):
        got = dec.align([x.T for x in utts], said, word_penalty=pen)
        score, pw, ps, pe, start = aref.align_batch(logb[:, order], lengths, indices, model["log_start"][order],
                                                    model["log_trans"][order], cases.log_exit(W, S), pen)
        woffs = np.r_[0, np.cumsum([len(t) for t in indices])]
        assert np.isfinite(score).all()
        for u, row in enumerate(got):
            segs = aref.segments(indices[u], start[woffs[u]:woffs[u + 1]], lengths[u])
            assert row["words"] == said[u] and len(row["segments"]) == len(said[u])
            assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
            assert np.array_equal(row["state_sequence"], ps[offs[u]:offs[u + 1]])
            rel = abs(row["log_likelihood"] - score[u]) / abs(score[u])
            worst = max(worst, rel)
            assert rel <= rtol
    print(f"Decoder.align {family}: max relative score difference {worst:.3g}")
    with pytest.raises(ValueError, match="'seven'"):
        dec.align([utts[0].T], [["zero", "seven"]])
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        dec.align([utts[0].T, utts[1].T], [["zero"]])
    # the other APIs of the same decoder still answer (the pack is shared, not consumed)
    assert len(dec.decode_connected([utts[0].T])) == 1


def test_decoder_align_refuses_custom_models(tmp_path):
    from sapr_amd.decoder import Decoder
    other = _pickle_models(tmp_path, "custom", [{"placeholder": "custom"}], ["zero"])
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=other, implementation="custom").align([np.zeros((13, 4), np.float32)], [["zero"]])


def test_word_examples_cut_the_utterances_at_the_boundaries():
    from sapr_amd.connected import connected_align
    seed, W, S, D, n = ref.E2E_CASES[3]
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    res = connected_align(utts, truth, _diag_network(model, 0.0))
    examples = res.word_examples(utts)
    assert sum(len(v) for v in examples.values()) == sum(len(t) for t in truth)
    assert sum(len(x) for v in examples.values() for x in v) == sum(len(x) for x in utts)
    for u, (x, words) in enumerate(zip(utts, truth)):
        segs = res.segments(u)
        assert len(segs) == len(words) and sum(b - a for _, a, b in segs) == len(x)
    for w, pieces in examples.items():
        assert len(pieces) == sum(t.count(w) for t in truth)
        assert all(p.ndim == 2 and p.shape[1] == D and len(p) >= S for p in pieces)
    u, (w, a, b) = 0, res.segments(0)[0]
    assert np.array_equal(examples[w][0], utts[u][a:b])
