"""Audio -> feature archive on the device: the counterpart of the reference's timit/steps/make_feat.sh, whose three Kaldi binaries
(compute-fbank-feats --config=conf/fbank.conf, compute-cmvn-stats, apply-cmvn --norm-vars=true with one global mean and variance) become
utils/features.Fbank and GlobalCMVN.  --feat-type mfcc is the recipe's feat_type=mfcc: compute-mfcc-feats --config=conf/mfcc.conf becomes
utils/features.Mfcc, --feat-type spectrogram is feat_type=spectrogram: compute-spectrogram-feats becomes utils/features.Spectrogram (257
columns under Kaldi's defaults), with the same global CMVN.  --feat-type logspec is the recipe's own local/make_spectrum.py
(utils/features.LogSpectrum): --conf holds `--key=value` lines after its audio_conf (sample-rate, window-size, window-stride, window,
normalize, input-scale; an empty file gives its defaults: 201 columns); it normalises every utterance by its own mean and standard
deviation, so every CMVN flag is refused.

    make_feat.py --conf fbank.conf --wav-scp train/wav.scp --out-dir DIR [--cmvn-stats FILE] [--compute-cmvn]
                 [--feat-type {fbank,mfcc,spectrogram,logspec}] [--speed-perturb 0.9,1.0,1.1] [--text FILE]
                 [--delta-order N [--delta-window W]]
                 [--utt2spk FILE | --cmvn-per-utt | --cmvn-sliding [--cmn-window N] [--min-cmn-window N] [--cmn-center]] [--norm-vars true|false]
                 [--reverb-copies N --rir-list FILE --noise-list FILE [--snrs 20,15,10,5,0] [--rir-prob P] [--noise-prob P] [--reverb-seed S]]
                 [--add-pitch [--pitch-conf FILE] [--pitch-process-conf FILE] [--paste-length-tolerance N]]

wav.scp: one `<utterance> <path>` per line (RIFF PCM-16 mono or uncompressed SPHERE; piped commands are not run).  Writes DIR/feats.ark and
DIR/feats.scp through write_kaldi_ark, utterances in wav.scp order: SpeechDataset and both drivers read them unchanged.
  --compute-cmvn   two passes: the first accumulates the global statistics on the device and writes them as Kaldi's text matrix
                   (--cmvn-stats, default DIR/global_<feat type>_cmvn.txt), the second writes features normalised with them (in the kernel)
  --cmvn-stats     without --compute-cmvn: statistics to apply (the training set's, for dev and test data); none: raw features
  --utt2spk        per-speaker CMVN, the normalisation of the standard Kaldi recipes (compute-cmvn-stats --spk2utt, apply-cmvn --utt2spk;
                   utils/features.SpeakerCMVN): FILE holds one `<utterance> <speaker>` per line; two passes over this list, the first
                   accumulates one statistics matrix per speaker on the device and writes them as Kaldi's text archive (--cmvn-stats,
                   default DIR/cmvn.ark.txt), the second normalises every utterance with its speaker's; DIR/utt2spk is written for the keys
                   of the archive.  A speed-perturbed or reverberated copy gets its speaker prefixed like its key (sp0.9-<speaker>,
                   rev1-<speaker>: Kaldi's convention), so copies never share statistics with the original
  --cmvn-per-utt   the same with every utterance its own speaker (apply-cmvn without --utt2spk)
  --cmvn-sliding   Kaldi's apply-cmvn-sliding (utils/features.SlidingCMVN) under its option names and defaults: --cmn-window 600,
                   --min-cmn-window 100, --cmn-center; one pass, no statistics file
  --norm-vars      for the three modes above: normalise the variance too; default true for speakers and utterances (the recipe's
                   apply-cmvn --norm-vars=true), false for the sliding window (Kaldi's default).  The three modes exclude each other,
                   --compute-cmvn and, except as the place to write the archive, --cmvn-stats
  --speed-perturb  Kaldi's speed perturbation (utils/perturb_data_dir_speed.sh): every utterance is written once per factor, under the key
                   sp<factor as typed>-<utterance>, in wav.scp order with the factors in the order given; factor f resamples on the device
                   from round(rate * f) to the configured rate (utils/features.SpeedPerturb), 1.0 resamples nothing; --compute-cmvn
                   accumulates over all copies
  --text           with --speed-perturb or --reverb-copies: the label file the loader reads (`<utterance> <labels>` lines), rewritten to DIR/text with the same
                   key prefixes -- SpeechDataset looks labels up by key, so a perturbed archive needs it
  --delta-order    Kaldi's add-deltas (its option names; --delta-window defaults to 2): N orders of delta features are appended to every frame,
                   13 cepstra becoming the usual 39 with N = 2.  As in Kaldi's pipelines they are taken AFTER the normalisation, from the
                   normalised base features, on the device (utils/features.FrameContext with no splice); the CMVN statistics are those of
                   the base features.  0 (the default): none
  --reverb-copies  multi-condition data (Kaldi's reverberate_data_dir.py / wav-reverberate; utils/features.Reverberate): next to every
                   utterance N copies with a room impulse response convolved in and background noise added, under the keys rev1-<utterance>
                   .. revN-<utterance> -- after resampling and speed perturbation, so rev1-sp0.9-<utterance> exists when both are on.
                   --rir-list / --noise-list (at least one): files naming one wave per line (`<path>` or `<name> <path>`, what read_wave
                   opens; resampled to the configured rate where they differ) on the scale of the data.  With probability --rir-prob
                   (default 1) one impulse response is convolved into a copy, with probability --noise-prob (default 1) one noise is
                   added at one of --snrs (dB, at most 16, default 20,15,10,5,0); a copy keeps its utterance's power and length.  The
                   draws are keyed by --reverb-seed and the copy's place in the length-sorted list, copy k continuing the count of
                   copy k - 1.  --text repeats the labels under the new keys; --compute-cmvn accumulates over the copies too
  --add-pitch      Kaldi's make_fbank_pitch.sh / make_mfcc_pitch.sh: the columns of compute-kaldi-pitch-feats | process-kaldi-pitch-feats
                   (utils/features.Pitch; three under Kaldi's defaults: 40 mel bins become 43 columns) pasted behind the base features
                   with paste-feats --length-tolerance=N (--paste-length-tolerance, default 2): both cut to the shorter frame count, an
                   error beyond the tolerance.  --pitch-conf / --pitch-process-conf: Kaldi's `--key=value` files for the two binaries;
                   without them Kaldi's defaults.  Pitch is taken from the waveform the base features see (resampled, perturbed,
                   reverberated) and its sample-frequency must be the base configuration's.  Every kind of CMVN is computed over and
                   applied to the pasted matrix, as in Kaldi's recipes, the statistics file holding all columns; deltas come behind it.
                   The noise on the delta-pitch column is keyed like the dither.  Refused with --feat-type logspec
A file whose sample rate differs from the configuration's is resampled on the device first (utils/features.Resampler, one plan per rate) when
the conf file holds Kaldi's --allow-downsample (file rate above the configured one) / --allow-upsample (below); otherwise it is an error.
Utterances are sorted by length and batched under --max-samples padded samples per launch.  Dither is the conf file's (Kaldi's default is
1.0; `--dither=0` in the conf switches it off), keyed by --seed and the utterance's place in the length-sorted list."""
import argparse
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from ctc_pytorch_amd.utils.data_loader import write_kaldi_ark  # noqa: E402
from ctc_pytorch_amd import frontend  # noqa: E402
from ctc_pytorch_amd.utils.features import (Fbank, FbankConfig, FrameContext, GlobalCMVN, LogSpecConfig, LogSpectrum, Mfcc, MfccConfig,  # noqa: E402
                                            Pitch, PitchConfig, ProcessPitchConfig, Reverberate, Spectrogram, Resampler, SlidingCMVN,
                                            SpeakerCMVN, SpectrogramConfig, paste_features, read_utt2spk, read_wave)

FEAT_TYPES = {"fbank": (FbankConfig, Fbank), "mfcc": (MfccConfig, Mfcc), "spectrogram": (SpectrogramConfig, Spectrogram),
              "logspec": (LogSpecConfig, LogSpectrum)}


def read_wav_scp(path):
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split(None, 1)
            if not parts:
                continue
            if len(parts) != 2 or parts[1].rstrip().endswith("|"):
                raise ValueError("%s:%d: expected '<utterance> <path>' (piped commands are not supported)" % (path, ln))
            out.append((parts[0], parts[1].strip()))
    return out


def length_batches(lengths, max_samples):
    """Index lists over the length-sorted utterances, each with B * max(length) <= max_samples (a single longer utterance stands alone)."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    batches, cur = [], []
    for i in order:                                                    # ascending: the newcomer is the batch's longest
        if cur and (len(cur) + 1) * max(lengths[i], 1) > max_samples:
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def parse_factors(text):
    """--speed-perturb's value: [(the factor as typed, its value)], in the order given."""
    out = []
    for part in text.split(","):
        part = part.strip()
        try:
            value = float(part)
        except ValueError:
            value = 0.0
        if not (value > 0.0 and value < float("inf")):
            raise ValueError("--speed-perturb: expected positive factors separated by commas (0.9,1.0,1.1), got %r" % text)
        out.append((part, value))
    if len(set(p for p, _ in out)) != len(out):
        raise ValueError("--speed-perturb: a factor is given twice in %r" % text)
    return out


def perturbed_keys(utts, factors):
    """The keys of a speed-perturbed list: every utterance once per factor as sp<factor as typed>-<utterance> (Kaldi's prefix), utterances in
    their order, the factors of one utterance in the order given.  `factors`: parse_factors' list, or None for the list as it is."""
    if factors is None:
        return list(utts)
    return ["sp%s-%s" % (typed, utt) for utt in utts for typed, _ in factors]


def perturb_text(lines, factors):
    """The lines of a label file (`<utterance> <labels>`) for perturbed_keys' list: every line once per factor, the key prefixed, the labels as
    they are.  Blank lines are dropped."""
    out = []
    for line in lines:
        parts = line.rstrip("\n").split(None, 1)
        if not parts:
            continue
        for key in perturbed_keys([parts[0]], factors):
            out.append(key + (" " + parts[1] if len(parts) > 1 else "") + "\n")
    return out


def parse_snrs(text):
    """--snrs' value: at most 16 finite numbers of dB, in the order given."""
    try:
        out = [float(part) for part in text.split(",")]
    except ValueError:
        out = []
    if not out or len(out) > 16 or any(v != v or abs(v) == float("inf") for v in out):
        raise ValueError("--snrs: expected 1 to 16 finite SNRs in dB separated by commas (20,15,10,5,0), got %r" % text)
    return out


def reverb_keys(keys, copies):
    """The keys of a list with reverberated copies: every key followed by rev1-<key> .. rev<copies>-<key>; 0 copies: the list as it is."""
    return [k for key in keys for k in [key] + ["rev%d-%s" % (c, key) for c in range(1, copies + 1)]]


def rewrite_text(lines, factors, copies):
    """The lines of a label file for the keys of the archive: perturb_text's lines, each followed by its reverberated copies' lines."""
    out = []
    for line in perturb_text(lines, factors):
        parts = line.rstrip("\n").split(None, 1)
        for key in reverb_keys([parts[0]], copies):
            out.append(key + (" " + parts[1] if len(parts) > 1 else "") + "\n")
    return out


def read_wave_list(path, target, device, max_samples):
    """The waves a list file names, one per line as `<path>` or `<name> <path>`, as arrays at `target` Hz: int16 as read, or float32 where
    the file's rate differs and the wave went through the Resampler."""
    paths = []
    with open(path) as f:
        for line in f:
            parts = line.split()
            if parts:
                paths.append(parts[-1])
    if not paths:
        raise ValueError("%s: no waves" % path)
    waves, rates = [], []
    for p in paths:
        samples, rate = read_wave(p)
        if samples.shape[0] < 1:
            raise ValueError("%s: %s holds no samples" % (path, p))
        waves.append(samples)
        rates.append(int(rate))
    if any(r != target for r in rates):
        waves = resample_waves(waves, rates, target, device, max_samples)
    return waves


def reverberate_waves(reverb, waves, copies, max_samples):
    """`copies` reverberated copies of every waveform: [copy 1 of all, copy 2 of all, ...] as float32 arrays, in length-sorted batches; the
    running utterance index of `reverb` follows the batches."""
    out = []
    batches = length_batches([w.shape[0] for w in waves], max_samples)
    for _ in range(copies):
        done = [None] * len(waves)
        for idx in batches:
            res, lens = reverb([waves[i] for i in idx])
            host = res.cpu().numpy()
            for b, i in enumerate(idx):
                done[i] = host[b, :lens[b]].copy()
        out.append(done)
    return out


def source_rate(utt, path, rate, config):
    """The rate a file is to be read at: its own, after the check of Kaldi's binaries -- a rate other than the configuration's needs
    allow_downsample (file rate higher) or allow_upsample (lower) in the configuration, else ValueError."""
    target = float(config.sample_frequency)
    if float(rate) == target:
        return int(rate)
    option = "allow_downsample" if rate > target else "allow_upsample"
    if not hasattr(config, option):
        raise ValueError("%s: %s is sampled at %d Hz, the configuration says %g (no resampling here)" % (utt, path, rate, config.sample_frequency))
    if not getattr(config, option):
        raise ValueError("%s: %s is sampled at %d Hz, the configuration says %g (no resampling here: --%s in --conf would allow it)"
                         % (utt, path, rate, config.sample_frequency, option.replace("_", "-")))
    if target != int(target):
        raise ValueError("%s: resampling needs a whole number of Hz as the configured rate, got %g" % (utt, config.sample_frequency))
    return int(rate)


def resample_waves(waves, source_rates, target, device, max_samples):
    """`waves` (int16 arrays) read at `source_rates` as waveforms at `target` Hz: those already there stay as they are, the others become
    float32 arrays, resampled on the device with one plan per source rate in length-sorted batches."""
    out = list(waves)
    for rate in sorted(set(source_rates) - {target}):
        idx = [i for i, r in enumerate(source_rates) if r == rate]
        resampler = Resampler(rate, target, device)
        for batch in length_batches([waves[i].shape[0] for i in idx], max_samples):
            res, lens = resampler([waves[idx[j]] for j in batch])
            host = res.cpu().numpy()
            for b, j in enumerate(batch):
                out[idx[j]] = host[b, :lens[b]].copy()
    return out


def copy_speakers(keys, bases, utt2spk):
    """The speaker of every key of the archive: the speaker of its base utterance behind the prefix the key carries in front of it
    (sp0.9-, rev1-, rev1-sp0.9-: Kaldi's convention for copies).  utt2spk None: every key is its own speaker."""
    if utt2spk is None:
        return list(keys)
    missing = [b for b in bases if b not in utt2spk]
    if missing:
        raise ValueError("--utt2spk names no speaker for %s" % missing[0])
    return [key[:len(key) - len(base)] + utt2spk[base] for key, base in zip(keys, bases)]


class PitchColumns(object):
    """--add-pitch: the pitch front-end, the tolerance of the paste and the normalisation of its columns.  cmvn: where a statistics pass
    accumulates the pitch columns (a GlobalCMVN or SpeakerCMVN of the front-end's feat_dim); stats: what the writing pass applies to them
    ((2, C + 1) or (G, 2, C + 1) float64 on the device, with `groups` the group of every index, or None)."""

    def __init__(self, front, tolerance):
        self.front, self.tolerance = front, int(tolerance)
        self.cmvn = self.stats = self.groups = None
        self.norm_vars = True

    def __call__(self, waves, seed, place):
        return self.front(waves, seed=seed, utt_offset=place)

    def normalised(self, pitch, frames, idx):
        if self.stats is None:
            return pitch
        groups = None if self.groups is None else [self.groups[i] for i in idx]
        return frontend.cmvn_apply(pitch, frames, self.stats, groups, norm_vars=self.norm_vars)


def joined_stats(base, pitch):
    """One Kaldi statistics matrix (or one per speaker) over the pasted columns from the two that were accumulated side by side over the
    same frames: sums of the base columns, sums of the pitch columns, the count."""
    a, b = base.stats.cpu(), pitch.stats.cpu()
    if not torch.equal(a[..., 0, -1], b[..., 0, -1]):
        raise RuntimeError("CMVN statistics of the base and the pitch columns were accumulated over different frame counts")
    return torch.cat([a[..., :-1], b[..., :-1], a[..., -1:]], dim=-1)


def make_features(fbank, waves, batches, mean=None, scale=None, seed=0, cmvn=None, deltas=None, speakers=None, normalise=None, pitch=None,
                  normalise_pasted=None):
    """Features of `waves` (list of int16 arrays), batch by batch: {index: (T, F) float32 ndarray}, or -- with `cmvn` -- nothing kept, the raw
    features accumulated into it (a SpeakerCMVN: under `speakers`, the speaker of every index).  normalise: called as (feats, frames,
    indices of the batch) on the features that are kept.  deltas (a FrameContext without splice or skip): applied behind it.  pitch (a
    PitchColumns): its columns are pasted behind the base features, both cut to the shorter frame count; statistics are accumulated over
    those frames, the pitch columns into pitch.cmvn; normalise_pasted: called like normalise on the pasted matrix."""
    mats, place = {}, 0
    for idx in batches:
        if isinstance(fbank, LogSpectrum):                             # normalised per utterance by the call itself; no dither
            feats, frames, _ = fbank([waves[i] for i in idx])
        else:
            feats, frames = fbank([waves[i] for i in idx], mean=mean, scale=scale, seed=seed, utt_offset=place)
        if pitch is not None:
            pcols, pframes = pitch([waves[i] for i in idx], seed, place)
            _, cut = paste_features(feats, frames, pcols, pframes, pitch.tolerance)    # (the tolerance, and the shorter counts)
        place += len(idx)
        if cmvn is not None:
            if pitch is not None:
                frames = cut
                if speakers is not None:
                    pitch.cmvn.accumulate(pcols, frames, [speakers[i] for i in idx])
                else:
                    pitch.cmvn.accumulate(pcols, frames)
            if speakers is not None:
                cmvn.accumulate(feats, frames, [speakers[i] for i in idx])
            else:
                cmvn.accumulate(feats, frames)
            continue
        if normalise is not None:
            feats = normalise(feats, frames, idx)
        if pitch is not None:
            feats, frames = paste_features(feats, cut, pitch.normalised(pcols, cut, idx), cut, 0)
            if normalise_pasted is not None:
                feats = normalise_pasted(feats, frames, idx)
        if deltas is not None:
            feats, frames, _ = deltas(feats, frames)
        host, n = feats.cpu().numpy(), frames.cpu().numpy()
        for b, i in enumerate(idx):
            mats[i] = host[b, :n[b]].copy()
    return mats


def parse_args(argv=None):
    """The command line, with the checks that need no file: the CMVN modes exclude each other."""
    ap = argparse.ArgumentParser(description="waveforms -> (normalised) filterbank features as a Kaldi archive, computed on the MI355X")
    ap.add_argument("--conf", required=True, help="Kaldi fbank config file (--key=value lines), e.g. the reference's conf/fbank.conf")
    ap.add_argument("--feat-type", choices=sorted(FEAT_TYPES), default="fbank", help="mfcc, spectrogram: --conf is read as that Kaldi config (conf/mfcc.conf, conf/spectrogram.conf); "
                    "logspec: the recipe's make_spectrum.py, --conf holds its audio_conf as --key=value lines, normalisation is per utterance")
    ap.add_argument("--wav-scp", required=True, help="list of '<utterance> <wav or sphere path>'")
    ap.add_argument("--out-dir", required=True, help="where feats.ark / feats.scp go")
    ap.add_argument("--cmvn-stats", default=None, help="Kaldi text CMVN statistics to apply (with --compute-cmvn: where to write them)")
    ap.add_argument("--compute-cmvn", action="store_true", help="accumulate global statistics over this list first, then normalise with them")
    ap.add_argument("--max-samples", type=int, default=32 * 8 * 16000, help="cap on padded samples per launch (default: 32 utterances of 8 s at 16 kHz)")
    ap.add_argument("--seed", type=int, default=0, help="dither seed")
    ap.add_argument("--speed-perturb", default=None, metavar="FACTORS", help="comma-separated speed factors (Kaldi's 0.9,1.0,1.1): every utterance "
                    "once per factor under the key sp<factor>-<utterance>")
    ap.add_argument("--text", default=None, help="with --speed-perturb or --reverb-copies: label file to rewrite to OUT_DIR/text with the new keys")
    ap.add_argument("--delta-order", type=int, default=0, help="append this many orders of delta features (Kaldi's add-deltas; 0: none)")
    ap.add_argument("--delta-window", type=int, default=2, help="add-deltas' window: the delta filter reaches this many frames to either side")
    ap.add_argument("--reverb-copies", type=int, default=None, metavar="N", help="write N reverberated / noisy copies of every utterance under "
                    "the keys rev<k>-<utterance> (needs --rir-list or --noise-list)")
    ap.add_argument("--rir-list", default=None, metavar="FILE", help="room impulse responses: one wave file per line")
    ap.add_argument("--noise-list", default=None, metavar="FILE", help="background noises: one wave file per line")
    ap.add_argument("--snrs", default=None, help="comma-separated SNRs in dB a noise is added at (default 20,15,10,5,0)")
    ap.add_argument("--rir-prob", type=float, default=None, help="probability that a copy is reverberated (default 1)")
    ap.add_argument("--noise-prob", type=float, default=None, help="probability that a copy gets noise (default 1)")
    ap.add_argument("--reverb-seed", type=int, default=None, help="seed of the copies' draws (default 0)")
    ap.add_argument("--utt2spk", default=None, metavar="FILE", help="per-speaker CMVN: '<utterance> <speaker>' lines; statistics per speaker are "
                    "accumulated over this list, written to --cmvn-stats (default OUT_DIR/cmvn.ark.txt) and applied")
    ap.add_argument("--cmvn-per-utt", action="store_true", help="per-utterance CMVN: every utterance is its own speaker")
    ap.add_argument("--cmvn-sliding", action="store_true", help="sliding-window CMVN (Kaldi's apply-cmvn-sliding)")
    ap.add_argument("--cmn-window", type=int, default=None, help="with --cmvn-sliding: window in frames (default 600)")
    ap.add_argument("--min-cmn-window", type=int, default=None, help="with --cmvn-sliding: smallest window at the start of an utterance (default 100)")
    ap.add_argument("--cmn-center", action="store_true", help="with --cmvn-sliding: centre the window on the frame")
    ap.add_argument("--norm-vars", choices=("true", "false"), default=None, help="with --utt2spk, --cmvn-per-utt (default true) or --cmvn-sliding "
                    "(default false): normalise the variance as well as the mean")
    ap.add_argument("--add-pitch", action="store_true", help="paste Kaldi's pitch columns (compute-kaldi-pitch-feats | process-kaldi-pitch-feats) "
                    "behind the base features")
    ap.add_argument("--pitch-conf", default=None, metavar="FILE", help="with --add-pitch: Kaldi config of compute-kaldi-pitch-feats (default: Kaldi's defaults)")
    ap.add_argument("--pitch-process-conf", default=None, metavar="FILE", help="with --add-pitch: Kaldi config of process-kaldi-pitch-feats "
                    "(default: Kaldi's defaults)")
    ap.add_argument("--paste-length-tolerance", type=int, default=None, metavar="N", help="with --add-pitch: paste-feats --length-tolerance (default 2)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)

    pitch_given = [n for n in ("pitch_conf", "pitch_process_conf", "paste_length_tolerance") if getattr(args, n) is not None]
    if pitch_given and not args.add_pitch:
        raise ValueError("--%s belongs to --add-pitch, which is not given" % pitch_given[0].replace("_", "-"))
    if args.add_pitch and args.feat_type == "logspec":
        raise ValueError("--add-pitch pastes Kaldi's pitch columns behind Kaldi's features: it does not apply to --feat-type logspec")
    if args.paste_length_tolerance is not None and args.paste_length_tolerance < 0:
        raise ValueError("--paste-length-tolerance takes a count of frames, got %d" % args.paste_length_tolerance)

    modes = [flag for flag, on in (("--utt2spk", args.utt2spk is not None), ("--cmvn-per-utt", args.cmvn_per_utt), ("--cmvn-sliding", args.cmvn_sliding),
                                   ("--compute-cmvn", args.compute_cmvn)) if on]
    if args.feat_type == "logspec" and (modes or args.cmvn_stats or args.norm_vars is not None):
        raise ValueError("--feat-type logspec normalises every utterance by its own mean and standard deviation (normalize in --conf): "
                         "--compute-cmvn, --cmvn-stats, --utt2spk, --cmvn-per-utt, --cmvn-sliding and --norm-vars do not apply to it")
    if len(modes) > 1:
        raise ValueError("%s and %s exclude each other: one normalisation per archive" % (modes[0], modes[1]))
    if args.cmvn_sliding and args.cmvn_stats:
        raise ValueError("--cmvn-sliding keeps no statistics: --cmvn-stats does not apply to it")
    sliding_given = [n for n in ("cmn_window", "min_cmn_window") if getattr(args, n) is not None] + (["cmn_center"] if args.cmn_center else [])
    if sliding_given and not args.cmvn_sliding:
        raise ValueError("--%s belongs to --cmvn-sliding, which is not given" % sliding_given[0].replace("_", "-"))
    if args.norm_vars is not None and not (args.utt2spk is not None or args.cmvn_per_utt or args.cmvn_sliding):
        raise ValueError("--norm-vars belongs to --utt2spk, --cmvn-per-utt or --cmvn-sliding; --compute-cmvn and --cmvn-stats always normalise the variance")
    args.cmn_window = 600 if args.cmn_window is None else args.cmn_window
    args.min_cmn_window = 100 if args.min_cmn_window is None else args.min_cmn_window
    if args.cmvn_sliding and (args.cmn_window < 1 or not 1 <= args.min_cmn_window <= args.cmn_window):
        raise ValueError("--cmn-window takes at least 1 and --min-cmn-window 1 to --cmn-window, got %d and %d" % (args.cmn_window, args.min_cmn_window))
    args.norm_vars = (not args.cmvn_sliding) if args.norm_vars is None else args.norm_vars == "true"
    return args


def main(argv=None, log=print):
    args = parse_args(argv)
    reverb_given = [n for n in ("rir_list", "noise_list", "snrs", "rir_prob", "noise_prob", "reverb_seed") if getattr(args, n) is not None]
    copies = args.reverb_copies or 0
    if args.reverb_copies is not None and args.reverb_copies < 1:
        raise ValueError("--reverb-copies takes a positive count, got %d" % args.reverb_copies)
    if copies and not (args.rir_list or args.noise_list):
        raise ValueError("--reverb-copies needs --rir-list or --noise-list")
    if reverb_given and not copies:
        raise ValueError("--%s belongs to --reverb-copies, which is not given" % reverb_given[0].replace("_", "-"))
    if args.snrs is not None and not args.noise_list:
        raise ValueError("--snrs belongs to --noise-list, which is not given")
    snrs = parse_snrs(args.snrs if args.snrs is not None else "20,15,10,5,0")
    rir_prob, noise_prob = (1.0 if p is None else p for p in (args.rir_prob, args.noise_prob))
    if not (0.0 <= rir_prob <= 1.0 and 0.0 <= noise_prob <= 1.0):
        raise ValueError("--rir-prob and --noise-prob are probabilities, got %g and %g" % (rir_prob, noise_prob))
    if args.text and not (args.speed_perturb or copies):
        raise ValueError("--text rewrites the label file for the keys of --speed-perturb or --reverb-copies: it needs one of them")
    if not 0 <= args.delta_order <= 2 or not 1 <= args.delta_window <= 5:
        raise ValueError("--delta-order takes 0, 1 or 2 and --delta-window 1 to 5, got %d and %d" % (args.delta_order, args.delta_window))
    deltas = FrameContext(delta_order=args.delta_order, delta_window=args.delta_window) if args.delta_order else None
    factors = parse_factors(args.speed_perturb) if args.speed_perturb else None
    config_type, frontend_type = FEAT_TYPES[args.feat_type]
    config = config_type.from_kaldi_conf(args.conf)
    device = torch.device(args.device)
    fbank = frontend_type(config, device)
    pitch = None
    if args.add_pitch:
        pitch_config = PitchConfig.from_kaldi_conf(args.pitch_conf) if args.pitch_conf else PitchConfig()
        process_config = ProcessPitchConfig.from_kaldi_conf(args.pitch_process_conf) if args.pitch_process_conf else ProcessPitchConfig()
        if float(pitch_config.sample_frequency) != float(config.sample_frequency):
            raise ValueError("--pitch-conf says %g Hz, --conf %g: both read the same waveform" % (pitch_config.sample_frequency, config.sample_frequency))
        pitch = PitchColumns(Pitch(pitch_config, process_config, device), 2 if args.paste_length_tolerance is None else args.paste_length_tolerance)
    pitch_dim = pitch.front.feat_dim if pitch is not None else 0
    entries = read_wav_scp(args.wav_scp)
    if not entries:
        raise ValueError("%s: no utterances" % args.wav_scp)
    bases = [utt for utt, _ in entries]                                # the utterance of wav.scp behind every key of the archive
    waves, rates = [], []
    for utt, path in entries:
        samples, rate = read_wave(path)
        waves.append(samples)
        rates.append(source_rate(utt, path, rate, config))
    if factors is not None:                                            # every utterance once per factor: the copies stand side by side
        if float(config.sample_frequency) != int(config.sample_frequency):
            raise ValueError("--speed-perturb needs a whole number of Hz as the configured rate, got %g" % config.sample_frequency)
        waves = [w for w in waves for _ in factors]
        rates = [int(round(r * f)) for r in rates for _, f in factors]
        entries = [(key, path) for utt, path in entries for key in perturbed_keys([utt], factors)]
        bases = [b for b in bases for _ in factors]
    if any(float(r) != float(config.sample_frequency) for r in rates):
        waves = resample_waves(waves, rates, int(config.sample_frequency), device, args.max_samples)
    if copies:                                                         # the copies stand behind their utterance
        rate = int(config.sample_frequency)
        if float(config.sample_frequency) != rate:
            raise ValueError("--reverb-copies needs a whole number of Hz as the configured rate, got %g" % config.sample_frequency)
        rirs = read_wave_list(args.rir_list, rate, device, args.max_samples) if args.rir_list else []
        noises = read_wave_list(args.noise_list, rate, device, args.max_samples) if args.noise_list else []
        reverb = Reverberate((rirs, noises, rate, snrs), rir_prob=rir_prob, noise_prob=noise_prob, seed=args.reverb_seed or 0, device=device)
        made = reverberate_waves(reverb, waves, copies, args.max_samples)
        waves = [w for i, clean in enumerate(waves) for w in [clean] + [made[c][i] for c in range(copies)]]
        entries = [(key, path) for utt, path in entries for key in reverb_keys([utt], copies)]
        bases = [b for b in bases for _ in range(copies + 1)]
        log("made %d reverberated copies of %d utterances from %d impulse responses and %d noises" % (copies, len(made[0]), len(rirs), len(noises)))
    batches = length_batches([w.shape[0] for w in waves], args.max_samples)
    os.makedirs(args.out_dir, exist_ok=True)

    mean = scale = normalise = normalise_pasted = None
    if args.utt2spk is not None or args.cmvn_per_utt:
        speakers = copy_speakers([key for key, _ in entries], bases, read_utt2spk(args.utt2spk) if args.utt2spk is not None else None)
        cmvn = SpeakerCMVN(fbank.feat_dim, sorted(set(speakers)), device)
        if pitch is not None:
            pitch.cmvn = SpeakerCMVN(pitch_dim, cmvn.speakers, device)
        make_features(fbank, waves, batches, seed=args.seed, cmvn=cmvn, speakers=speakers, pitch=pitch)
        stats_path = args.cmvn_stats or os.path.join(args.out_dir, "cmvn.ark.txt")
        written = cmvn
        if pitch is not None:                                          # one matrix per speaker over the pasted columns, as Kaldi writes it
            written = SpeakerCMVN(fbank.feat_dim + pitch_dim, cmvn.speakers)
            written.stats.copy_(joined_stats(cmvn, pitch.cmvn))
            pitch.stats, pitch.groups, pitch.norm_vars = pitch.cmvn.stats, [cmvn.index[s] for s in speakers], args.norm_vars
        written.save_kaldi_text(stats_path)
        log("wrote CMVN statistics of %d speakers to %s" % (len(cmvn.speakers), stats_path))
        if args.utt2spk is not None:
            with open(os.path.join(args.out_dir, "utt2spk"), "w") as f:
                f.writelines("%s %s\n" % (key, spk) for (key, _), spk in zip(entries, speakers))

        def normalise(feats, frames, idx):
            return cmvn.apply(feats, frames, [speakers[i] for i in idx], norm_vars=args.norm_vars, out=feats)
    elif args.cmvn_sliding:
        sliding = SlidingCMVN(args.cmn_window, args.min_cmn_window, normalize_variance=args.norm_vars, center=args.cmn_center)

        def slide(feats, frames, idx):
            return sliding(feats, frames)
        normalise, normalise_pasted = (slide, None) if pitch is None else (None, slide)      # over the pasted matrix, column by column
    elif args.compute_cmvn:
        cmvn = GlobalCMVN(fbank.feat_dim, device)
        if pitch is not None:
            pitch.cmvn = GlobalCMVN(pitch_dim, device)
        make_features(fbank, waves, batches, seed=args.seed, cmvn=cmvn, pitch=pitch)
        stats_path = args.cmvn_stats or os.path.join(args.out_dir, "global_%s_cmvn.txt" % args.feat_type)
        written = cmvn
        if pitch is not None:
            written = GlobalCMVN(fbank.feat_dim + pitch_dim)
            written.stats.copy_(joined_stats(cmvn, pitch.cmvn))
            pitch.stats = pitch.cmvn.stats
        written.save_kaldi_text(stats_path)
        log("wrote CMVN statistics of %d frames to %s" % (int(cmvn.stats[0, -1].item()), stats_path))
        mean, scale = cmvn.mean_scale(device)
    elif args.cmvn_stats:
        cmvn = GlobalCMVN.load_kaldi_text(args.cmvn_stats)
        if cmvn.feat_dim != fbank.feat_dim + pitch_dim:
            raise ValueError("%s holds statistics of %d dimensions, the configuration gives %d" % (args.cmvn_stats, cmvn.feat_dim,
                                                                                                 fbank.feat_dim + pitch_dim))
        if pitch is not None:                                          # the matrix over the pasted columns: base sums | pitch sums | count
            F = fbank.feat_dim
            pitch.stats = torch.cat([cmvn.stats[:, F:-1], cmvn.stats[:, -1:]], dim=1).contiguous().to(device)
            base = GlobalCMVN(F)
            base.stats.copy_(torch.cat([cmvn.stats[:, :F], cmvn.stats[:, -1:]], dim=1))
            cmvn = base
        mean, scale = cmvn.mean_scale(device)
    mats = make_features(fbank, waves, batches, mean=mean, scale=scale, seed=args.seed, deltas=deltas, normalise=normalise, pitch=pitch,
                         normalise_pasted=normalise_pasted)
    ark, scp = os.path.join(args.out_dir, "feats.ark"), os.path.join(args.out_dir, "feats.scp")
    write_kaldi_ark(ark, scp, {utt: mats[i] for i, (utt, _) in enumerate(entries)})
    out_dim = fbank.feat_dim + pitch_dim
    log("wrote %d utterances, %d frames of %d dimensions to %s" % (len(entries), sum(m.shape[0] for m in mats.values()),
                                                                          out_dim if deltas is None else deltas.out_dim(out_dim), ark))
    if args.text:
        with open(args.text) as f:
            lines = rewrite_text(f.readlines(), factors, copies)
        with open(os.path.join(args.out_dir, "text"), "w") as f:
            f.writelines(lines)
        log("wrote %d label lines to %s" % (len(lines), os.path.join(args.out_dir, "text")))
    return ark, scp


if __name__ == "__main__":
    main()
