"""GPU: online connected-word decoding (csrc/connected_online.hip) through the Python layer against the CPU restatement
tests/_online_ref.py, which is the definition, push by push, and against the device's own offline decoder at the end.
The recursion is float64 adds and compares only and the walks read bytes: every comparison is ``np.array_equal``."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import _bigram_ref as bref
from tests import _connected_family_cases as fam
from tests import _connected_ref as ref
from tests import _online_cases as cases
from tests import _online_ref as oref

pytestmark = pytest.mark.gpu

# the shapes and lengths of tests/test_bigram_gpu.py: all nine (RL, SP) instantiations; 9 streams, not a multiple of
# the 4 a workgroup serves
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (25, 10), (64, 4), (5, 7), (2, 1),
          (3, 12), (17, 3), (4, 11)]
LENGTHS = [3, 40, 1, 65, 0, 17, 2, 64, 33]
ROWS = ("path_word", "path_state", "path_entry")


def _net(tabs, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(*tabs, bigram=WordBigram(*lm))


def _split(logb, lengths):
    offs = np.r_[0, np.cumsum(lengths)]
    return [logb[a:b] for a, b in zip(offs[:-1], offs[1:])]


def _assert_update(got, want, what):
    assert (got.first_frame, len(got.path_word), got.frames, got.stable_frames, got.forced) == \
        (want.first_frame, want.n_new, want.frames, want.stable_frames, want.forced), what
    for f in ROWS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)


def _assert_result(got, want, what):
    _assert_update(got.update, want, what)
    assert np.float64(got.score).tobytes() == np.float64(want.score).tobytes(), what
    assert (got.n_words, got.forced) == (want.n_words, want.forced), what


def _plans(name, rng, max_chunk):
    if name == "each":
        return [[1] * T for T in LENGTHS]
    if name == "seven":
        return [cases.fixed_chunks(T, 7) for T in LENGTHS]
    return [cases.ragged_chunks(rng, T, max_chunk) for T in LENGTHS]


def _drive(ses, model, utts, plans, hypothesis=False):
    """Push the utterances chunk by chunk into the device session and the restatement, comparing every push; a stream
    is finished at the push after its last chunk.  Returns the device's ``OnlineResult`` per stream."""
    at, step, done = [0] * len(utts), [0] * len(utts), {}
    while len(done) < len(utts):
        chunks = []
        for u, x in enumerate(utts):
            n = plans[u][step[u]] if step[u] < len(plans[u]) else 0
            chunks.append(x[at[u]:at[u] + n] if u not in done else None)
            at[u] += n
            step[u] += 1
        got = ses.push(logb=chunks, hypothesis=hypothesis)
        want = model.push(chunks, want_hyp=hypothesis)
        for u in range(len(utts)):
            _assert_update(got[u], want[u], (u, step[u]))
            if hypothesis:
                for a, b in zip(got[u].hypothesis_rows, want[u].hyp):
                    assert np.array_equal(a, b), (u, step[u])
        ended = [u for u in range(len(utts)) if u not in done and step[u] >= len(plans[u])]
        if ended:
            for u, g, w in zip(ended, ses.finish(ended), model.finish(ended)):
                _assert_result(g, w, ("finish", u))
                done[u] = g
    return [done[u] for u in range(len(utts))]


def _assert_offline(results, offline, lengths, what):
    """Where nothing was forced and the score is finite the concatenation is the offline decoder's."""
    offs = np.r_[0, np.cumsum(lengths)]
    for u, r in enumerate(results):
        assert np.float64(r.score).tobytes() == offline.score[u:u + 1].tobytes(), (what, u)
        if r.forced == 0 and np.isfinite(r.score):
            assert r.n_words == offline.n_words[u], (what, u)
            for f in ROWS:
                assert np.array_equal(getattr(r, f), getattr(offline, f)[offs[u]:offs[u + 1]]), (what, u, f)


@pytest.mark.parametrize("chunking", ["each", "seven", "ragged"])
@pytest.mark.parametrize("topology,exits", [("dense", "any"), ("bidiag", "last")])
@pytest.mark.parametrize("W,S", SHAPES)
def test_every_push_equals_the_restatement(W, S, topology, exits, chunking):
    """``window = 64, max_chunk = 8``: the 64- and 65-frame streams of the bidiagonal case, which never settle, are
    forced as well."""
    from sapr_amd.connected import ConnectedSession, connected_viterbi
    tabs, lm, logb = cases.random_case(W, S, topology, exits, sum(LENGTHS))
    net = _net(tabs, lm)
    ses = ConnectedSession(net, len(LENGTHS), window=64, max_chunk=8)
    model = oref.Session(*tabs, *lm, len(LENGTHS), 64, 8)
    plans = _plans(chunking, np.random.default_rng(W * S), 8)
    results = _drive(ses, model, _split(logb, LENGTHS), plans)
    _assert_offline(results, connected_viterbi(logb, LENGTHS, net), LENGTHS, (W, S, topology, exits, chunking))
    empty = results[LENGTHS.index(0)]
    assert empty.score == -np.inf and empty.n_words == 0 and len(empty.path_word) == 0
    if exits == "any" and W > 2:
        assert all(r.forced == 0 and len(r.path_word) == T for r, T in zip(results, LENGTHS))


@pytest.mark.parametrize("window", [16, 64])
def test_a_small_window_forces_and_keeps_the_score(window):
    from sapr_amd.connected import ConnectedSession, connected_viterbi
    tabs, lm, logb = cases.forcing_case()
    net = _net(tabs, lm)
    ses = ConnectedSession(net, 1, window=window, max_chunk=7)
    model = oref.Session(*tabs, *lm, 1, window, 7)
    res = _drive(ses, model, [logb], [cases.fixed_chunks(150, 7)])[0]
    assert res.forced > 0 and len(res.path_word) == 150
    assert np.float64(res.score).tobytes() == connected_viterbi(logb, [150], net).score.tobytes()


def _two_rounds(ses, first, second, order):
    """Stream ``order[k]`` decodes ``first[k]`` and then, from the push after its end, ``second[k]`` — while its
    neighbours are mid-utterance.  Chunks of 5 frames.  Returns ``[(result of first, result of second)]`` by k."""
    B = len(order)
    queue = [[(0, first[k]), (1, second[k])] for k in range(B)]
    at, out = [0] * B, [[None, None] for _ in range(B)]
    while any(queue):
        chunks = [None] * B
        for k in range(B):
            if queue[k]:
                x = queue[k][0][1]
                chunks[order[k]] = x[at[k]:at[k] + 5]
                at[k] += 5
        ses.push(logb=chunks)
        ended = [k for k in range(B) if queue[k] and at[k] >= len(queue[k][0][1])]
        for k, r in zip(ended, ses.finish([order[k] for k in ended])):
            out[k][queue[k].pop(0)[0]] = r
            at[k] = 0
    return out


def test_streams_are_reused_isolated_and_repeatable():
    """Thirteen streams (not a multiple of the four a workgroup serves), two utterances each."""
    from sapr_amd.connected import ConnectedSession, connected_viterbi
    B = 13
    rng = np.random.default_rng(5)
    len1, len2 = rng.integers(1, 60, B).tolist(), rng.integers(1, 60, B).tolist()
    tabs, lm, logb = cases.random_case(11, 10, "dense", "any", sum(len1) + sum(len2))
    net = _net(tabs, lm)
    first, second = _split(logb[:sum(len1)], len1), _split(logb[sum(len1):], len2)
    off1 = connected_viterbi(logb[:sum(len1)], len1, net)
    off2 = connected_viterbi(logb[sum(len1):], len2, net)
    ses = ConnectedSession(net, B, window=64, max_chunk=5)
    a = _two_rounds(ses, first, second, list(range(B)))
    _assert_offline([r[0] for r in a], off1, len1, "first")
    _assert_offline([r[1] for r in a], off2, len2, "second")
    assert all(r.forced == 0 for pair in a for r in pair)
    perm = rng.permutation(B).tolist()
    for other in (_two_rounds(ses, first, second, list(range(B))),             # the same bytes again
                  _two_rounds(ConnectedSession(net, B, window=64, max_chunk=5), first, second, perm)):
        for x, y in zip(a, other):
            for r, q in zip(x, y):
                assert np.float64(r.score).tobytes() == np.float64(q.score).tobytes() and r.n_words == q.n_words
                for f in ROWS:
                    assert getattr(r, f).tobytes() == getattr(q, f).tobytes(), f
    # an abandoned recording: the reset byte makes stream 6 fresh while its neighbours carry on
    for u in range(B):
        ses.push(logb=[first[v][:5] for v in range(B)])
    ses.reset([6])
    ses.push(logb=[second[6][:5] if v == 6 else None for v in range(B)])
    ses.push(logb=[second[6][5:10] if v == 6 else None for v in range(B)])
    r = ses.finish([6])[0]
    want = connected_viterbi(second[6][:10], [len(second[6][:10])], net)
    _assert_offline([r], want, [len(second[6][:10])], "reset")
    assert len(r.path_word) == len(second[6][:10])


def test_the_hypothesis_is_what_a_flush_would_write():
    from sapr_amd.connected import ConnectedSession
    tabs, lm, logbs, _, _ = cases.e2e_case(3)
    utts = [logbs[u] for u in cases.two_longest(logbs)] + [logbs[0][:0]]
    net = _net(tabs, lm)
    ses = ConnectedSession(net, 3, window=64, max_chunk=7)
    model = oref.Session(*tabs, *lm, 3, 64, 7)
    ups, segments = None, [[], [], []]
    for a in range(0, max(len(x) for x in utts), 7):
        chunks = [x[a:a + 7] for x in utts]
        ups = ses.push(logb=chunks, hypothesis=True)
        for u, (g, w) in enumerate(zip(ups, model.push(chunks, want_hyp=True))):
            _assert_update(g, w, a)
            for x, y in zip(g.hypothesis_rows, w.hyp):
                assert np.array_equal(x, y), a
            segments[u] += g.segments
    res = ses.finish()
    for u, (up, r) in enumerate(zip(ups, res)):
        assert segments[u] + r.update.segments == r.segments()  # every segment is handed out once, when it is complete
        assert len(up.hypothesis_rows[0]) == up.frames - up.stable_frames
        for x, f in zip(up.hypothesis_rows, ROWS):
            assert np.array_equal(x, getattr(r.update, f)), f
    assert len(ups[0].hypothesis_rows[0]) > 0 and ups[0].hypothesis == r_words(ups[0], res[0])
    assert ups[2].hypothesis == [] and res[2].score == -np.inf


def r_words(up, res):
    """The words of ``res`` that lie, wholly or in part, in the frames that were pending at ``up``."""
    return [w for w, a, b in res.segments() if b > up.stable_frames]


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def _abi(W, S, window, B):
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    rc = lib.sapr_connected_online_state_bytes(B, W, S, window, C.byref(n))
    return lib, _lib, torch, rc, int(n.value)


def test_c_abi_truncates_an_over_long_chunk_and_refuses_bad_arguments():
    W, S, window, max_chunk, T = 5, 7, 32, 6, 10
    lib, _lib, torch, rc, nbytes = _abi(W, S, window, 1)
    assert rc == 0 and nbytes > 0
    tabs, lm, logb = cases.random_case(W, S, "dense", "any", T)
    net = _net(tabs, lm)
    dev = _lib.require_gpu()
    ls, lt, lx, _ = net.device(dev)
    dlm = net.device_lm(dev)
    rows = torch.full((T, net.R), float("-inf"), dtype=torch.float64, device=dev).reshape(T, W, net.SP)
    rows[:, :, :S] = torch.from_numpy(logb).to(dev)
    rows = rows.reshape(T, net.R).contiguous()
    offs = torch.tensor([0, T], dtype=torch.int64, device=dev)
    state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    trunc = torch.zeros(1, dtype=torch.uint8, device=dev)
    p, cs = _lib.ptr, _lib.current_stream

    def step(state_bytes=nbytes, lm_ptr=p(dlm[0]), w=W, s=S, win=window, mc=max_chunk):
        return lib.sapr_connected_online_step(p(rows), p(offs), 1, T, p(ls), p(lt), p(lx), lm_ptr, p(dlm[1]),
                                              p(dlm[2]), w, s, win, mc, p(state), state_bytes, None, p(trunc), cs())

    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    assert step(state_bytes=nbytes - 1) == ERR_ARG          # a short state buffer
    assert step(lm_ptr=None) == ERR_ARG                     # a NULL pointer
    assert step(mc=window) == ERR_ARG and step(mc=0) == ERR_ARG and step(win=1, mc=1) == ERR_ARG
    assert step(w=0) == ERR_ARG
    assert step(w=15, s=18) == ERR_UNSUPPORTED              # W * SP = 270 > 256
    assert lib.sapr_connected_online_state_bytes(1, 15, 18, window, C.byref(C.c_size_t(0))) == ERR_UNSUPPORTED
    assert lib.sapr_connected_online_state_bytes(1, W, S, window, None) == ERR_ARG
    torch.cuda.synchronize()
    assert not state.any()                                  # refused before any launch
    assert step() == 0
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    n_new, first, forced = i32(1), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64,
                                                                                            device=dev)
    ow, os_, oe = i32(1, window), i32(1, window), torch.zeros((1, window), dtype=torch.uint8, device=dev)
    score, n_words = torch.zeros(1, dtype=torch.float64, device=dev), i32(1)
    flush = torch.ones(1, dtype=torch.uint8, device=dev)

    def commit(state_bytes=nbytes, out=p(ow), fl=p(flush), sc=p(score)):
        return lib.sapr_connected_online_commit(1, W, S, window, max_chunk, p(state), state_bytes, fl, p(n_new),
                                                p(first), out, p(os_), p(oe), sc, p(n_words), p(forced), None, None,
                                                None, None, cs())

    assert commit(state_bytes=8) == ERR_ARG and commit(out=None) == ERR_ARG and commit(sc=None) == ERR_ARG
    assert commit() == 0
    torch.cuda.synchronize()
    assert trunc.item() == 1
    assert (first.item(), n_new.item(), forced.item()) == (0, max_chunk, 0)     # max_chunk frames were consumed
    want = bref.viterbi(logb[:max_chunk], *tabs, *lm)
    assert np.float64(score.item()).tobytes() == np.float64(want[0]).tobytes() and n_words.item() == want[1]
    assert np.array_equal(ow[0, :max_chunk].cpu().numpy(), want[2])
    assert lib.sapr_connected_online_step(None, None, 0, 0, None, None, None, p(dlm[0]), p(dlm[1]), p(dlm[2]), W, S,
                                          window, max_chunk, None, 0, None, None, cs()) == 0     # n_streams == 0


def test_push_refuses_an_over_long_chunk_by_name():
    from sapr_amd.connected import ConnectedSession
    tabs, lm, logb = cases.random_case(5, 7, "dense", "any", 12)
    ses = ConnectedSession(_net(tabs, lm), 2, window=16, max_chunk=4)
    with pytest.raises(ValueError, match="stream 1"):
        ses.push(logb=[logb[:4], logb[:5]])
    with pytest.raises(ValueError):
        ConnectedSession(_net(tabs, lm), 2, window=4, max_chunk=4)


# ---- end to end: Decoder.open_connected against Decoder.decode_connected -------------------------------------------
def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def _online_equals_offline(dec, utts, net_family, chunk=10, **kw):
    """``open_connected`` in chunks of ``chunk`` frames against ``decode_connected``: first the emission of a chunk is
    byte-equal to the same rows of the whole-utterance emission, then the dicts are equal."""
    import torch
    from sapr_amd import connected
    net = dec._connected_network("last", 0.0)
    assert net.family == net_family
    emit = connected._EMIT[net.family]
    whole = emit(torch.from_numpy(np.concatenate(utts)).cuda(), net).cpu().numpy()
    offs = np.r_[0, np.cumsum([len(x) for x in utts])]
    for a in (0, chunk, 2 * chunk):      # the chunk rows of every stream, packed as a push packs them
        packed = np.concatenate([x[a:a + chunk] for x in utts])
        if len(packed) == 0:
            continue
        part = emit(torch.from_numpy(packed).cuda(), net).cpu().numpy()
        same = np.concatenate([whole[lo + a:min(lo + a + chunk, hi)] for lo, hi in zip(offs[:-1], offs[1:])])
        assert part.tobytes() == same.tobytes(), a
    feats = [x.T for x in utts]
    want = dec.decode_connected(feats, **kw)
    ses = dec.open_connected(len(utts), window=256, max_chunk=chunk, **kw)
    seen = [[] for _ in utts]
    for a in range(0, max(len(x) for x in utts), chunk):
        for u, row in enumerate(ses.push([f[:, a:a + chunk] for f in feats])):
            seen[u] += row["segments"]
    got = ses.finish()
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.pop("forced") == 0
        assert np.float64(g["log_likelihood"]).tobytes() == np.float64(w["log_likelihood"]).tobytes(), u
        assert g["words"] == w["words"] and g["segments"] == w["segments"], u
        assert g["state_sequence"].dtype == w["state_sequence"].dtype
        assert np.array_equal(g["state_sequence"], w["state_sequence"]), u
        assert seen[u] == w["segments"][:len(seen[u])], u      # what the pushes handed out, in order
    assert any(seen)
    return want


def test_decoder_session_equals_decode_connected(tmp_path):
    from sapr_amd.connected import WordBigram
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    seed, W, S, D, n = ref.E2E_CASES[0]
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    models = []
    for w in range(W):
        m = GaussianHMM(n_components=S, covariance_type="diag")
        m.means_, m._covars_ = model["means"][w], model["vars"][w]
        m.startprob_, m.transmat_ = model["startprob"][w], model["transmat"][w]
        models.append(m)
    names = [f"w{w:02d}" for w in range(W)]
    dec = Decoder(models_dir=_pickle_models(tmp_path, "hmmlearn", models, names), implementation="hmmlearn", n_iter=15)
    pos = [dec.vocab.index(nm) for nm in names]
    bigram = WordBigram.from_transcripts([[pos[w] for w in t] for t in truth], W)
    want = _online_equals_offline(dec, utts, "diag", bigram=bigram, word_penalty=-2.0)
    assert all(np.isfinite(row["log_likelihood"]) and row["words"] for row in want)
    with pytest.raises(ValueError, match="stream 3"):
        dec.open_connected(4, max_chunk=10).push([None, None, None, utts[0].T[:, :11]])


@pytest.mark.parametrize("family,impl,spec", [("gmm", "gmmhmm", fam.GMM_DECODER_CASE),
                                              ("full", "hmmlearn", fam.FULL_DECODER_CASE)])
def test_decoder_session_serves_the_other_emission_families(tmp_path, family, impl, spec):
    from sapr_amd.decoder import Decoder
    model, utts, _ = fam.case(family, spec)
    names = ["zero", "one", "two", "three"]
    dec = Decoder(models_dir=_pickle_models(tmp_path, impl, fam.models_of(family, model), names), implementation=impl,
                  n_iter=15)
    _online_equals_offline(dec, list(utts), family)


def test_custom_models_are_refused(tmp_path):
    from sapr_amd.decoder import Decoder
    root = _pickle_models(tmp_path, "custom", [object()], ["zero"])
    with pytest.raises(ValueError, match="custom"):
        Decoder(models_dir=root, implementation="custom", n_iter=15).open_connected(1)
