"""Reverberation and additive noise on the HIP kernels (ctcn_reverb) through the C entry point, ops.reverberate, utils/features.Reverberate
and steps/make_feat.py (--reverb-copies), against the numpy restatement of tests/reverb_ref.py and the host twin.  The demand is
bit-identity: every sum has a fixed order and every float64 operation is rounded on its own (include/ctcn.h).  The cases -- lengths around
a tile, impulse responses around a tap chunk, both clamps of the early window, short, long and all-zero noises -- are
test_reverb_host.CASES."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_ref as RV  # noqa: E402
from test_reverb_host import CASES, SEED, SNRS, TILE, bits, built, near_end_seed, noise, rir, want, write_wav  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -54321.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def poisoned(batch, lens, spare=3):
    """The batch with `spare` more columns and, behind every utterance's length, NaN (float32) or the largest sample (int16)."""
    out = np.zeros((batch.shape[0], batch.shape[1] + spare), dtype=batch.dtype)
    out[:] = np.nan if batch.dtype == np.float32 else 32767
    for b, n in enumerate(lens):
        out[b, :n] = batch[b, :n]
    return out


_POISONED_BANKS = {}


def poisoned_bank(bank, dev):
    """A device copy of the bank block with NaN in every float word behind a row's length (the builder leaves zeros there): what the
    kernels get as bank_dev, so a read behind K_r or L_m shows in the output.  The tables' places come from the block's header."""
    key = (id(bank), str(dev))
    if key not in _POISONED_BANKS:
        words = bank.host.copy()
        hdr, f = words.view(np.int32), words.view(np.float32)
        assert int(hdr[1]) == bank.R and int(hdr[2]) == bank.N and int(hdr[12]) == words.shape[0]
        rirs = int(hdr[11])
        noises = rirs + bank.R * bank.rir_stride
        assert noises + bank.N * bank.noise_stride == words.shape[0]
        poisoned = 0
        for r in range(bank.R):
            K = int(bank.rir_meta[r][0])
            assert not np.any(f[rirs + r * bank.rir_stride + K:rirs + (r + 1) * bank.rir_stride])      # the builder's zeros
            f[rirs + r * bank.rir_stride + K:rirs + (r + 1) * bank.rir_stride] = np.nan
            poisoned += bank.rir_stride - K
        for m in range(bank.N):
            n = int(bank.noise_len[m])
            f[noises + m * bank.noise_stride + n:noises + (m + 1) * bank.noise_stride] = np.nan
            poisoned += bank.noise_stride - n
        assert int(np.isnan(f[rirs:]).sum()) == poisoned
        _POISONED_BANKS[key] = (bank, torch.from_numpy(words.view(np.int32)).to(dev), poisoned)
    return _POISONED_BANKS[key][1:]


def run_raw(bank, batch, lens, dev, utt_offset=3, seed=SEED, rir_prob=1.0, noise_prob=1.0, normalize=True):
    """ctcn_reverb called directly on a poisoned batch with a poisoned bank block, the output pre-filled with a sentinel."""
    L = _lib.lib()
    bank_dev, _ = poisoned_bank(bank, dev)
    x = poisoned(batch, lens)
    w = torch.from_numpy(x).to(dev)
    B, Nmax = x.shape
    out = torch.full((B, Nmax), SENTINEL, dtype=torch.float32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    need = L.ctcn_reverb_ws_bytes(bank._host_ptr(), B, Nmax)
    ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    o = _lib.ReverbOpts(rir_prob=rir_prob, noise_prob=noise_prob, normalize=int(normalize))
    _lib.check(L.ctcn_reverb(p(w), int(x.dtype == np.int16), p(lens_d), bank._host_ptr(), p(bank_dev), ctypes.byref(o), seed, utt_offset, p(out),
                             B, Nmax, p(ws), ws.numel() * 8, _lib.stream_ptr()), "reverb")
    return out.cpu().numpy()


def check_rows(out, wanted, lens, what):
    assert not np.any(out == SENTINEL), "elements left unwritten"
    assert not np.isnan(out).any(), "NaN from behind a length reached the output"
    for b, n in enumerate(lens):
        assert np.all(bits(out[b, n:]) == 0), (what, b, n)                # zeros (+0.0) from the utterance's length on
        assert np.array_equal(bits(out[b, :n]), bits(wanted[b])), (what, b, n, int((bits(out[b, :n]) != bits(wanted[b])).sum()))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_are_the_restatement_and_the_host_twin_bit_for_bit(name, normalize, dev):
    bank, _, batch, lens = built(name)
    out = run_raw(bank, batch, lens, dev, normalize=normalize)
    check_rows(out, want(name, normalize=normalize), lens, name)
    twin = [ops.reverberate_host(batch[b, :n], bank, SEED, 3 + b, normalize=normalize) for b, n in enumerate(lens)]
    check_rows(out, twin, lens, name + " (host twin)")


@pytest.mark.parametrize("name", ["banks", "ragged_banks"])
def test_nothing_behind_a_bank_row_is_read(name, dev):
    """The block the kernels read holds NaN behind every row's length (hundreds of words in these banks), every row of both lists is
    drawn by some utterance, and the output is the restatement's: no NaN, bit for bit."""
    bank, ref, batch, lens = built(name)
    _, poisoned = poisoned_bank(bank, dev)
    assert poisoned >= 1000
    plans = [RV.plan(ref, SEED, 3 + b) for b, n in enumerate(lens) if n]
    assert {pl["rir"] for pl in plans} == set(range(bank.R)) and len({pl["noise"] for pl in plans}) >= 2, plans
    for normalize in (True, False):
        out = run_raw(bank, batch, lens, dev, normalize=normalize)
        check_rows(out, want(name, normalize=normalize), lens, name)


@pytest.mark.parametrize("probs", [(1.0, 0.0), (0.0, 1.0), (0.5, 0.5)])
def test_parts_switched_off_or_drawn(probs, dev):
    bank, ref, batch, lens = built("banks")
    for normalize in (True, False):
        out = run_raw(bank, batch, lens, dev, utt_offset=40, seed=5, rir_prob=probs[0], noise_prob=probs[1], normalize=normalize)
        check_rows(out, [RV.reverberate(batch[b, :n], ref, 5, 40 + b, probs[0], probs[1], normalize) for b, n in enumerate(lens)], lens, probs)


def test_both_parts_off_keep_the_input_bits(dev):
    for name in ("banks", "tile_edges_f32"):
        bank, _, batch, lens = built(name)
        for normalize in (True, False):
            out = run_raw(bank, batch, lens, dev, rir_prob=0.0, noise_prob=0.0, normalize=normalize)
            check_rows(out, [batch[b, :n].astype(np.float32) for b, n in enumerate(lens)], lens, name)


def test_noise_wraps_from_an_offset_near_its_end(dev):
    bank, ref, batch, lens = built("chunk_minus_1")
    seed = near_end_seed(bank, 0, 7, slack=0)
    assert ops.reverb_plan(bank, seed, 0)["offset"] == 6 and ops.reverb_plan(bank, seed, 0)["noise"] == 0
    out = run_raw(bank, batch, lens, dev, utt_offset=0, seed=seed)
    check_rows(out, [RV.reverberate(batch[b, :n], ref, seed, b) for b, n in enumerate(lens)], lens, "offset 6 of 7")


def test_a_row_alone_is_its_row_in_the_batch(dev):
    bank, _, batch, lens = built("banks")
    whole = run_raw(bank, batch, lens, dev)
    for b, n in enumerate(lens):
        alone = run_raw(bank, batch[b:b + 1, :max(n, 1)], [n], dev, utt_offset=3 + b)
        assert np.array_equal(bits(alone[0, :n]), bits(whole[b, :n])), b


def test_ops_and_the_features_class(dev):
    bank, ref, batch, lens = built("banks")
    w = torch.from_numpy(batch).to(dev)
    a = ops.reverberate(w, lens, bank, SEED, utt_offset=3)
    assert a.shape == w.shape and a.dtype == torch.float32
    check_rows(a.cpu().numpy(), want("banks", normalize=True), lens, "ops")
    again = ops.reverberate(w, torch.tensor(lens, device=dev), bank, SEED, utt_offset=3)
    assert torch.equal(a, again)                                        # the same seed: the same bits
    other = ops.reverberate(w, lens, bank, SEED + 1, utt_offset=3)
    assert not torch.equal(a, other)
    assert [ops.reverb_plan(bank, SEED, 3 + b) for b in range(7)] != [ops.reverb_plan(bank, SEED + 1, 3 + b) for b in range(7)]
    rirs, noises, fs, _, _ = CASES["banks"]
    r = features.Reverberate((rirs, noises, fs, SNRS), seed=SEED, device=dev, start_index=3)
    assert r.plan(4) == RV.plan(ref, SEED, 4)
    first, l1 = r([batch[b, :n] for b, n in enumerate(lens)])
    assert l1 == lens and r.index == 3 + len(lens)
    check_rows(first.cpu().numpy(), want("banks", normalize=True), lens, "Reverberate")
    second, _ = r(w, lens)                                              # the running index moved on: other draws
    assert r.index == 3 + 2 * len(lens) and not torch.equal(first, second)
    third, _ = r(w, lens, utt_offset=3)
    assert torch.equal(third, first) and r.index == 3 + 2 * len(lens)
    with pytest.raises(TypeError):
        ops.reverberate(w.double(), lens, bank, 1)
    with pytest.raises(ValueError):
        ops.reverberate(w, lens[:-1], bank, 1)
    with pytest.raises(RuntimeError, match="probability"):
        ops.reverberate(w, lens, bank, 1, rir_prob=1.5)


def test_rows_beyond_two_to_the_31_elements(dev):
    """Three rows of 2^30 samples (the longest the call takes): the third starts at element 2^31 of the batch and of the output, where a
    32-bit index would wrap.  Only that row holds an utterance; the rest of 12.9 GB comes out as zeros.  Needs 19 GB of device memory
    (6.4 GB of int16 input, 12.9 GB of output) for 0.34 s, measured alone; a run short of memory leaves it out with
    -k "not two_to_the_31"."""
    bank, ref, batch, lens = built("tile_edges")
    Nmax, n = 1 << 30, lens[2]
    w = torch.zeros((3, Nmax), dtype=torch.int16, device=dev)
    w[2, :n] = torch.from_numpy(batch[2, :n]).to(dev)
    w[1, :5] = 32767                                                    # behind a length of 0: never read
    out = ops.reverberate(w, [0, 0, n], bank, SEED, utt_offset=3)
    assert tuple(out.shape) == (3, Nmax)
    assert np.array_equal(bits(out[2, :n].cpu().numpy()), bits(want("tile_edges", normalize=True)[2]))
    assert int(torch.count_nonzero(out[0])) == 0 and int(torch.count_nonzero(out[1])) == 0 and int(torch.count_nonzero(out[2, n:])) == 0
    del w, out
    torch.cuda.empty_cache()


def test_make_feat_reverb_copies_end_to_end(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    rs = np.random.RandomState(3)
    utts = {"spk_a": 9000, "spk_b": 4100, "spk_c": 6000}
    with open(tmp_path / "wav.scp", "w") as f:
        for utt, n in utts.items():
            write_wav(tmp_path / (utt + ".wav"), rs.randint(-9000, 9001, size=n))
            f.write("%s %s\n" % (utt, tmp_path / (utt + ".wav")))
    write_wav(tmp_path / "h0.wav", (rir(300, 20, 4) / 4 * 32000).astype(np.int16))
    write_wav(tmp_path / "h1.wav", (rir(500, 10, 5) / 4 * 32000).astype(np.int16), rate=8000)       # resampled to 16 kHz
    write_wav(tmp_path / "q0.wav", noise(5000, 6, 2000.0).astype(np.int16))
    (tmp_path / "rirs.txt").write_text("%s\n%s\n" % (tmp_path / "h0.wav", tmp_path / "h1.wav"))
    (tmp_path / "noises.txt").write_text("n0 %s\n" % (tmp_path / "q0.wav"))
    (tmp_path / "fbank.conf").write_text("--num-mel-bins=23\n--dither=0\n")
    (tmp_path / "text").write_text("spk_a sil a sil\nspk_b sil b\nspk_c c\n")
    common = ["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp"), "--device", str(dev)]
    quiet = lambda *_: None                                              # noqa: E731

    ark0, scp0 = make_feat.main(common + ["--out-dir", str(tmp_path / "plain")], log=quiet)
    reverb = ["--rir-list", str(tmp_path / "rirs.txt"), "--noise-list", str(tmp_path / "noises.txt"), "--snrs", "15,5", "--reverb-copies", "2",
              "--reverb-seed", "11"]
    log = []
    ark, scp = make_feat.main(common + ["--out-dir", str(tmp_path / "rev"), "--text", str(tmp_path / "text")] + reverb, log=log.append)
    keys = [line.split()[0] for line in open(scp)]
    assert keys == ["spk_a", "rev1-spk_a", "rev2-spk_a", "spk_b", "rev1-spk_b", "rev2-spk_b", "spk_c", "rev1-spk_c", "rev2-spk_c"]
    assert open(tmp_path / "rev" / "text").read().splitlines() == [
        "spk_a sil a sil", "rev1-spk_a sil a sil", "rev2-spk_a sil a sil", "spk_b sil b", "rev1-spk_b sil b", "rev2-spk_b sil b",
        "spk_c c", "rev1-spk_c c", "rev2-spk_c c"]
    mats = {line.split()[0]: read_kaldi_matrix(line.split()[1]) for line in open(scp)}
    plain = {line.split()[0]: read_kaldi_matrix(line.split()[1]) for line in open(scp0)}
    for utt in utts:
        assert np.array_equal(mats[utt], plain[utt])                    # the clean data stands as it was
        for k in (1, 2):
            m = mats["rev%d-%s" % (k, utt)]
            assert m.shape == plain[utt].shape and np.isfinite(m).all() and not np.array_equal(m, plain[utt])
        assert not np.array_equal(mats["rev1-" + utt], mats["rev2-" + utt])
    assert any("2 reverberated copies of 3 utterances from 2 impulse responses and 1 noises" in s for s in log)

    # with speed perturbation: the copies are copies of the perturbed data
    _, scp2 = make_feat.main(common + ["--out-dir", str(tmp_path / "both"), "--speed-perturb", "0.9,1.0", "--rir-list", str(tmp_path / "rirs.txt"),
                                       "--reverb-copies", "1", "--text", str(tmp_path / "text")], log=quiet)
    keys2 = [line.split()[0] for line in open(scp2)]
    assert keys2[:4] == ["sp0.9-spk_a", "rev1-sp0.9-spk_a", "sp1.0-spk_a", "rev1-sp1.0-spk_a"] and len(keys2) == 12
    assert open(tmp_path / "both" / "text").read().splitlines()[:2] == ["sp0.9-spk_a sil a sil", "rev1-sp0.9-spk_a sil a sil"]

    # without the options: the bytes of the path that knows nothing of them
    config = features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf"))
    fbank = features.Fbank(config, dev)
    waves = [features.read_wave(str(tmp_path / (utt + ".wav")))[0] for utt in utts]
    old = make_feat.make_features(fbank, waves, make_feat.length_batches([w.shape[0] for w in waves], 32 * 8 * 16000))
    from ctc_pytorch_amd.utils.data_loader import write_kaldi_ark
    os.makedirs(tmp_path / "old")
    write_kaldi_ark(str(tmp_path / "old" / "feats.ark"), str(tmp_path / "old" / "feats.scp"), {utt: old[i] for i, utt in enumerate(utts)})
    assert open(ark0, "rb").read() == open(tmp_path / "old" / "feats.ark", "rb").read()
    assert not os.path.exists(tmp_path / "plain" / "text")
