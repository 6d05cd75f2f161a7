"""Waveform -> normalised filterbank features on the device: the stage in front of utils/data_loader.py.  Counterpart of the three Kaldi
binaries of the reference's timit/steps/make_feat.sh (compute-fbank-feats --config=conf/fbank.conf, compute-cmvn-stats, apply-cmvn
--norm-vars=true with one global mean and variance); steps/make_feat.py is the driver.

  FbankConfig   Kaldi's option names and defaults; from_kaldi_conf reads a `--key=value` file such as the reference's conf/fbank.conf
  Fbank         the configured front-end on one device (frontend.fbank behind it; holds the uploaded plan)
  MfccConfig    the same for compute-mfcc-feats (the recipe's feat_type=mfcc, conf/mfcc.conf): Kaldi's MFCC defaults, use_energy = true
  Mfcc          the MFCC front-end (frontend.mfcc: the same kernel with the DCT, the lifter and Kaldi's column rules behind its log-mel stage)
  SpectrogramConfig / Spectrogram   compute-spectrogram-feats (the recipe's feat_type=spectrogram): the log power of every FFT bin, the log
                energy in column 0 (frontend.spectrogram: the same kernel without the mel bank)
  LogSpecConfig / LogSpectrum       the recipe's own spectrogram (local/make_spectrum.py: a centred STFT of 400 points, log1p of the magnitude,
                one mean and standard deviation per utterance; frontend.log_spectrum)
  GlobalCMVN    Kaldi's 2 x (F + 1) statistics, accumulated on the device (frontend.cmvn_accumulate), its text file, mean and 1 / stddev
  SpeakerCMVN   the same statistics per speaker (compute-cmvn-stats --spk2utt, apply-cmvn --utt2spk; one speaker per utterance: per-utterance
                CMVN), accumulated and applied on the device (frontend.cmvn_accumulate_groups, frontend.cmvn_apply), its text archive; read_utt2spk
  SlidingCMVN   Kaldi's apply-cmvn-sliding (frontend.cmvn_sliding): normalisation over a running window, for data without speaker labels
  Resampler     a waveform batch at another sample rate (frontend.resample: Kaldi's LinearResample, what its binaries run under --allow-downsample /
                --allow-upsample); SpeedPerturb: the recipe's three-way speed perturbation (perturb_data_dir_speed.sh) as one Resampler per factor
  FrameContext  the stage behind them: Kaldi's add-deltas, frame splicing, frame skipping and the pad to a multiple of n_downsample on the
                device (frontend.frame_context) -- what utils/data_loader.py does per utterance on the host; its output is the model's input
  SpecAugment   the online augmentation between the two: time warp, frequency masks and time masks of the base batch (frontend.spec_augment),
                redrawn for every utterance of every epoch from (seed, running utterance index)
  Reverberate   multi-condition data on the waveform, in front of any of the front-ends: a room impulse response convolved into the utterance
                and background noise added at a drawn SNR (frontend.reverberate; Kaldi's wav-reverberate), drawn from (seed, running index)
  PitchConfig / ProcessPitchConfig / Pitch   Kaldi's pitch features (compute-kaldi-pitch-feats, process-kaldi-pitch-feats: frontend.pitch,
                frontend.pitch_process): NCCF over geometric lags, a Viterbi search, the probability of voicing; three columns under the defaults.
                paste_features: paste-feats --length-tolerance, the `fbank + pitch` of Kaldi's make_fbank_pitch.sh
  read_wave     RIFF PCM-16 mono and uncompressed NIST SPHERE (TIMIT's) -> int16 samples

Not here: VTLN, compressed SPHERE, online (chunked) pitch."""
import struct

import numpy as np
import torch

from .. import _lib, frontend

WINDOW_TYPES = ("hamming", "hanning", "povey", "rectangular", "blackman")     # the order of ctcn_fbank_opts.window_type
LOGSPEC_WINDOWS = ("hamming", "hann", "blackman", "bartlett")                  # the order of ctcn_logspec_opts.window


class _KaldiConfig(object):
    """What the config classes share: options under Kaldi's names (dashes as underscores) held as attributes, converted to the types
    of the class's DEFAULTS, and the reader of Kaldi's `--key=value` files.  DEFAULTS holds the options of the feature computation itself;
    DRIVER_OPTIONS those of Kaldi's binaries around it (allow_downsample, allow_upsample: what to do with a file at another sample rate),
    read and kept the same way, acted on by steps/make_feat.py and absent from the C structs."""
    DEFAULTS = {}
    DRIVER_OPTIONS = dict(allow_downsample=False, allow_upsample=False)

    @classmethod
    def _options(cls):
        return dict(cls.DEFAULTS, **cls.DRIVER_OPTIONS)

    def __init__(self, **kw):
        name = type(self).__name__
        options = self._options()
        for k in kw:
            if k not in options:
                raise ValueError("%s: unknown option %r" % (name, k))
        for k, d in options.items():
            setattr(self, k, self._convert(k, kw.get(k, d)))
        self._check_window()

    def _check_window(self):
        if self.window_type not in WINDOW_TYPES:
            raise ValueError("%s: unknown window type %r (one of %s)" % (type(self).__name__, self.window_type, ", ".join(WINDOW_TYPES)))

    @classmethod
    def _convert(cls, key, value):
        d = cls._options()[key]
        if isinstance(d, bool):
            if isinstance(value, str):
                if value.lower() not in ("true", "false", "t", "f", "1", "0"):
                    raise ValueError("%s: %s expects true or false, got %r" % (cls.__name__, key, value))
                return value.lower() in ("true", "t", "1")
            return bool(value)
        return type(d)(value)

    @classmethod
    def from_kaldi_conf(cls, path):
        """A Kaldi config file: one `--key=value` per line, a bare `--flag` means true, `#` starts a comment, blank lines are skipped.
        A key this front-end does not implement raises ValueError (a silently ignored option would change the features)."""
        kw = {}
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                line = line.split("#", 1)[0].strip()
                if not line:
                    continue
                if not line.startswith("--"):
                    raise ValueError("%s:%d: expected --key=value, got %r" % (path, ln, line))
                key, _, value = line[2:].partition("=")
                key = key.strip().replace("-", "_")
                if key not in cls._options():
                    raise ValueError("%s:%d: unknown or unsupported option --%s" % (path, ln, key.replace("_", "-")))
                kw[key] = value.strip() if _ else "true"
        return cls(**kw)

    def _frame_mel_opts(self):
        """The fields ctcn_fbank_opts and ctcn_mfcc_opts have in common."""
        return dict(samp_freq=self.sample_frequency, frame_shift_ms=self.frame_shift, frame_length_ms=self.frame_length,
                    preemph_coeff=self.preemphasis_coefficient, blackman_coeff=self.blackman_coeff, low_freq=self.low_freq,
                    high_freq=self.high_freq, energy_floor=self.energy_floor, window_type=WINDOW_TYPES.index(self.window_type),
                    num_mel_bins=self.num_mel_bins, remove_dc_offset=self.remove_dc_offset,
                    round_to_power_of_two=self.round_to_power_of_two, snip_edges=self.snip_edges, use_energy=self.use_energy,
                    raw_energy=self.raw_energy, htk_compat=self.htk_compat)


class FbankConfig(_KaldiConfig):
    """The options of Kaldi's compute-fbank-feats that the kernel implements, under Kaldi's names (dashes as underscores) and with Kaldi's
    defaults -- dither = 1.0 among them: pass dither=0 for a deterministic front-end.  allow_downsample / allow_upsample (Kaldi's, here
    and in MfccConfig and SpectrogramConfig; both false, in DRIVER_OPTIONS) let steps/make_feat.py resample a file recorded at a higher /
    lower rate to sample_frequency first (Resampler); they are not options of the kernel and do not enter the C struct."""
    DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                    remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                    num_mel_bins=23, low_freq=20.0, high_freq=0.0, use_energy=False, energy_floor=0.0, raw_energy=True, htk_compat=False,
                    use_log_fbank=True, use_power=True)

    @property
    def feat_dim(self):
        return self.num_mel_bins + (1 if self.use_energy else 0)

    def c_opts(self):
        return _lib.FbankOpts(use_log_fbank=self.use_log_fbank, use_power=self.use_power, **self._frame_mel_opts())


class MfccConfig(_KaldiConfig):
    """The options of Kaldi's compute-mfcc-feats, under Kaldi's names and with Kaldi's MFCC defaults: use_energy is TRUE here (the
    reference's conf/mfcc.conf switches it off), and there is no use_log_fbank / use_power -- an MFCC is always taken from the log of the
    mel-filtered power spectrum, and those keys are unknown options."""
    DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                    remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                    num_mel_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13, use_energy=True, energy_floor=0.0, raw_energy=True,
                    cepstral_lifter=22.0, htk_compat=False)

    @property
    def feat_dim(self):
        return self.num_ceps

    def c_opts(self):
        return _lib.MfccOpts(num_ceps=self.num_ceps, cepstral_lifter=self.cepstral_lifter, **self._frame_mel_opts())


class SpectrogramConfig(_KaldiConfig):
    """The options of Kaldi's compute-spectrogram-feats, under Kaldi's names and with Kaldi's defaults: the frame options, energy_floor,
    raw_energy and return_raw_fft -- read and kept, but true is refused when the plan is built (Kaldi's complex output is not built).
    There is no mel bank: num_mel_bins and the frequency limits are unknown options."""
    DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                    remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                    energy_floor=0.0, raw_energy=True, return_raw_fft=False)

    @property
    def feat_dim(self):
        L = int(float(np.float32(self.sample_frequency)) * 0.001 * float(np.float32(self.frame_length)))
        return (1 << (L - 1).bit_length()) // 2 + 1

    def c_opts(self):
        return _lib.SpectrogramOpts(samp_freq=self.sample_frequency, frame_shift_ms=self.frame_shift, frame_length_ms=self.frame_length,
                                    preemph_coeff=self.preemphasis_coefficient, blackman_coeff=self.blackman_coeff,
                                    energy_floor=self.energy_floor, window_type=WINDOW_TYPES.index(self.window_type),
                                    remove_dc_offset=self.remove_dc_offset, round_to_power_of_two=self.round_to_power_of_two,
                                    snip_edges=self.snip_edges, raw_energy=self.raw_energy, return_raw_fft=self.return_raw_fft)


class LogSpecConfig(_KaldiConfig):
    """The audio_conf of the recipe's local/make_spectrum.py under its own names and defaults, plus normalize (its parse_audio argument) and
    input_scale (multiplied onto the samples first: log1p is not scale-free, and the reference's loader may hand floats in +-1 where
    read_wave hands the int16 range).  n_fft = int(sample_rate * window_size), hop = int(sample_rate * window_stride).  from_kaldi_conf
    reads the same `--key=value` lines (`--window-size=0.032`); an empty file gives the defaults."""
    DEFAULTS = dict(sample_rate=16000.0, window_size=0.025, window_stride=0.01, window="hamming", normalize=True, input_scale=1.0)
    DRIVER_OPTIONS = {}                                                # (make_spectrum.py has no rate options: a mismatch stays an error)

    def _check_window(self):
        if self.window not in LOGSPEC_WINDOWS:
            raise ValueError("LogSpecConfig: unknown window %r (one of %s)" % (self.window, ", ".join(LOGSPEC_WINDOWS)))

    @property
    def sample_frequency(self):
        return self.sample_rate

    @property
    def n_fft(self):
        return int(self.sample_rate * self.window_size)

    @property
    def hop(self):
        return int(self.sample_rate * self.window_stride)

    @property
    def feat_dim(self):
        return self.n_fft // 2 + 1

    def c_opts(self):
        return _lib.LogSpecOpts(sample_rate=self.sample_rate, window_size=self.window_size, window_stride=self.window_stride,
                                input_scale=self.input_scale, window=LOGSPEC_WINDOWS.index(self.window), normalize=self.normalize)


def _batch(name, waves, lengths):
    """(padded (B, Nmax) int16 / float32 tensor, lengths) of a list of 1-D waveforms, or of a padded batch with `lengths`."""
    if lengths is None:
        arrs = [w.cpu().numpy() if torch.is_tensor(w) else np.asarray(w) for w in waves]
        if not arrs or any(a.ndim != 1 for a in arrs):
            raise ValueError("%s: expected a non-empty list of 1-D waveforms" % name)
        lengths = [a.shape[0] for a in arrs]
        batch = np.zeros((len(arrs), max(max(lengths), 1)), dtype=np.int16 if all(a.dtype == np.int16 for a in arrs) else np.float32)
        for b, a in enumerate(arrs):
            batch[b, :a.shape[0]] = a
        waves = torch.from_numpy(batch)
    elif not torch.is_tensor(waves):
        waves = torch.from_numpy(np.ascontiguousarray(waves))
    if waves.dtype not in (torch.int16, torch.float32):
        waves = waves.to(torch.float32)
    return waves, lengths


class _FrontEnd(object):
    """A configured front-end on one device: the plan (built here, so a configuration outside the kernel's range raises RuntimeError here)
    and the call that batches waveforms for the kernel.  Subclasses name the plan type and the op."""
    _plan_type = None
    _op = None

    def __init__(self, config, device):
        self.config = config
        self.device = torch.device(device)
        self.plan = self._plan_type(config.c_opts())
        self.feat_dim = self.plan.feat_dim

    def num_frames(self, num_samples):
        return self.plan.num_frames(num_samples)

    def __call__(self, waves, lengths=None, mean=None, scale=None, seed=0, utt_offset=0):
        """waves: a list of 1-D waveforms (int16 or float arrays / tensors on Kaldi's scale: int16 range), or a padded (B, Nmax) batch with
        `lengths`.  mean / scale: the (F) vectors of GlobalCMVN.mean_scale, applied by the same kernel.  Returns (feats (B, Tmax, F) float32
        zero-padded, frames (B) int32) on the device: the loader's layout.  Dither is config.dither, keyed by (seed, b + utt_offset)."""
        waves, lengths = _batch(type(self).__name__, waves, lengths)
        vec = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).to(self.device)
        return type(self)._op(waves.to(self.device), lengths, self.plan, mean=vec(mean), scale=vec(scale), dither=self.config.dither, seed=seed,
                              utt_offset=utt_offset)


class Fbank(_FrontEnd):
    """The filterbank front-end of one FbankConfig on one device.  Building it builds the plan: a configuration outside the kernel's range (a
    padded frame other than 256 / 512 / 1024 samples, more than 128 mel bins, round_to_power_of_two=false) raises RuntimeError here."""
    _plan_type = frontend.FbankPlan
    _op = staticmethod(frontend.fbank)


class Mfcc(_FrontEnd):
    """The MFCC front-end of one MfccConfig on one device: Fbank's call signature and return layout with F = num_ceps.  Beyond Fbank's
    limits, num_ceps outside [1, num_mel_bins], more than 64 cepstra or a negative lifter raise RuntimeError here."""
    _plan_type = frontend.MfccPlan
    _op = staticmethod(frontend.mfcc)


class Spectrogram(_FrontEnd):
    """The spectrogram front-end of one SpectrogramConfig on one device: Fbank's call signature and return layout with F = Npad / 2 + 1
    (257 under the defaults).  A padded frame other than 256 / 512 / 1024 samples, round_to_power_of_two=false or return_raw_fft=true raise
    RuntimeError here."""
    _plan_type = frontend.SpectrogramPlan
    _op = staticmethod(frontend.spectrogram)


class LogSpectrum(object):
    """The recipe's own spectrogram of one LogSpecConfig on one device (frontend.log_spectrum).  Building it builds the plan: an n_fft other than
    256, 400, 512 or 1024 raises RuntimeError here.  Normalisation is per utterance and part of the call; there is no mean / scale."""

    def __init__(self, config, device):
        self.config = config
        self.device = torch.device(device)
        self.plan = frontend.LogSpecPlan(config.c_opts())
        self.feat_dim = self.plan.feat_dim

    def num_frames(self, num_samples):
        return self.plan.num_frames(num_samples)

    def __call__(self, waves, lengths=None):
        """waves as Fbank takes them.  Returns (feats (B, Tmax, F) float32 zero-padded, frames (B) int32, stats (B, 2) float32: the mean and
        standard deviation of each utterance) on the device."""
        waves, lengths = _batch("LogSpectrum", waves, lengths)
        return frontend.log_spectrum(waves.to(self.device), lengths, self.plan)


class PitchConfig(_KaldiConfig):
    """The options of Kaldi's compute-kaldi-pitch-feats (PitchExtractionOptions) under Kaldi's names and with Kaldi's defaults.  The offline
    computation only: the chunking and latency options of the online extractor are unknown options.  snip_edges=false, a preemphasis and
    what else the kernels do not take are read and kept, and refused when the plan is built."""
    DEFAULTS = dict(frontend.PITCH_OPTIONS)
    DRIVER_OPTIONS = {}

    def _check_window(self):
        pass

    def plan(self):
        return frontend.PitchPlan(**{k: getattr(self, k) for k in self.DEFAULTS})


class ProcessPitchConfig(_KaldiConfig):
    """The options of Kaldi's process-kaldi-pitch-feats (ProcessPitchOptions) under Kaldi's names and with Kaldi's defaults: three columns
    (POV feature, normalised log pitch, delta log pitch).  A delay other than 0 is read and kept, and refused at the first call."""
    DEFAULTS = dict(frontend.PITCH_PROCESS_OPTIONS)
    DRIVER_OPTIONS = {}

    def _check_window(self):
        pass

    @property
    def feat_dim(self):
        return sum(bool(getattr(self, k)) for k in ("add_pov_feature", "add_normalized_log_pitch", "add_delta_pitch", "add_raw_log_pitch"))

    def kw(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


class Pitch(object):
    """Kaldi's pitch features of one PitchConfig and one ProcessPitchConfig on one device (frontend.pitch, frontend.pitch_process; Kaldi's
    make_fbank_pitch.sh pipes the same two binaries).  Building it builds the plan: a configuration outside the kernels' range raises
    RuntimeError here.  feat_dim: 3 under the defaults."""

    def __init__(self, config=None, process_config=None, device="cuda:0"):
        self.config = config if config is not None else PitchConfig()
        self.process_config = process_config if process_config is not None else ProcessPitchConfig()
        self.device = torch.device(device)
        self.plan = self.config.plan()
        self.feat_dim = self.process_config.feat_dim
        if self.feat_dim == 0:
            raise ValueError("Pitch: every column of the post-processing is switched off")
        if self.process_config.delay != 0:
            raise RuntimeError("Pitch: a delay other than 0 is not built")

    def num_frames(self, num_samples):
        return self.plan.num_frames(num_samples)

    def raw(self, waves, lengths=None):
        """compute-kaldi-pitch-feats alone: (raw (B, Tmax, 2) float32: NCCF and pitch in Hz, frames (B) int32)."""
        waves, lengths = _batch("Pitch", waves, lengths)
        return frontend.pitch(waves.to(self.device), lengths, self.plan)

    def __call__(self, waves, lengths=None, seed=0, utt_offset=0):
        """waves as Fbank takes them, at config.sample_frequency.  Returns (feats (B, Tmax, feat_dim) float32 zero-padded, frames (B)
        int32) on the device.  The noise on the delta column is keyed by (seed, b + utt_offset), as Fbank's dither."""
        raw, frames = self.raw(waves, lengths)
        return frontend.pitch_process(raw, frames, seed=seed, utt_offset=utt_offset, **self.process_config.kw()), frames


def paste_features(a, frames_a, b, frames_b, length_tolerance=2):
    """Kaldi's paste-feats --length-tolerance on two zero-padded device batches of the same utterances: a (B, Ta, Fa), b (B, Tb, Fb) float32
    with their frame counts (lists or tensors) -> (out (B, T, Fa + Fb) float32, frames (B) int32): both cut to the shorter frame count of
    every utterance, rows beyond it zero.  ValueError where the counts of an utterance differ by more than length_tolerance."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device:
        raise ValueError("paste_features: expected two float32 batches (B, T, F) of the same B on one device")
    fa = [int(v) for v in (frames_a.tolist() if torch.is_tensor(frames_a) else frames_a)]
    fb = [int(v) for v in (frames_b.tolist() if torch.is_tensor(frames_b) else frames_b)]
    B = a.shape[0]
    if len(fa) != B or len(fb) != B:
        raise ValueError("paste_features: %d and %d frame counts for a batch of %d" % (len(fa), len(fb), B))
    for i, (x, y) in enumerate(zip(fa, fb)):
        if abs(x - y) > int(length_tolerance):
            raise ValueError("paste_features: utterance %d has %d and %d frames, more than the tolerance of %d apart" % (i, x, y, int(length_tolerance)))
        if not (0 <= x <= a.shape[1] and 0 <= y <= b.shape[1]):
            raise ValueError("paste_features: frame counts %d and %d of utterance %d outside the batches" % (x, y, i))
    frames = torch.tensor([min(x, y) for x, y in zip(fa, fb)], dtype=torch.int32)
    T = int(frames.max()) if B else 0
    frames = frames.to(a.device)
    out = torch.cat([a[:, :T], b[:, :T]], dim=2)
    keep = torch.arange(T, device=a.device)[None, :] < frames[:, None]
    return torch.where(keep[:, :, None], out, torch.zeros((), dtype=out.dtype, device=out.device)), frames


class Resampler(object):
    """Waveforms at orig_freq Hz -> new_freq Hz on one device (frontend.resample: Kaldi's LinearResample with ResampleWaveform's parameters: a
    Hann-windowed sinc of lowpass_filter_width zero crossings, cutoff = cutoff_ratio * 0.5 * min(rates)).  Building it builds the plan: a
    pair of rates whose filter table does not fit the kernel's LDS budget raises RuntimeError here.  Equal rates build nothing and pass the
    batch through."""

    def __init__(self, orig_freq, new_freq, device, lowpass_filter_width=6, cutoff_ratio=0.99):
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
            raise ValueError("Resampler: sample rates must be whole numbers of Hz, got %r -> %r" % (orig_freq, new_freq))
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.device = torch.device(device)
        self.plan = None
        if self.orig_freq != self.new_freq:
            self.plan = frontend.ResamplePlan(self.orig_freq, self.new_freq, num_zeros=lowpass_filter_width,
                                         cutoff=cutoff_ratio * 0.5 * min(self.orig_freq, self.new_freq))

    def num_samples(self, num_samples):
        return int(num_samples) if self.plan is None else self.plan.num_samples(num_samples)

    def __call__(self, waves, lengths=None):
        """waves as Fbank takes them.  Returns (out (B, Mmax) float32 zero-padded on the device, lengths list): any front-end's (waves, lengths)
        form.  Samples stay on the input's scale.  Equal rates: the batch as it came (int16 stays int16), moved to the device."""
        waves, lengths = _batch("Resampler", waves, lengths)
        waves = waves.to(self.device)
        if self.plan is None:
            return waves, [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        return frontend.resample(waves, lengths, self.plan)


class SpeedPerturb(object):
    """Kaldi's speed perturbation (utils/perturb_data_dir_speed.sh: sox `speed f`, factors 0.9 / 1.0 / 1.1) at one sample rate: perturbing by
    f is resampling from round(sample_frequency * f) to sample_frequency and reading the result at sample_frequency -- ceil(n / f) samples,
    pitch and tempo both scaled by f.  One Resampler per factor, built here; factor 1.0 is the identity."""

    def __init__(self, sample_frequency, factors=(0.9, 1.0, 1.1), device="cuda:0"):
        if int(sample_frequency) != sample_frequency:
            raise ValueError("SpeedPerturb: the sample rate must be a whole number of Hz, got %r" % (sample_frequency,))
        self.sample_frequency = int(sample_frequency)
        self.factors = tuple(float(f) for f in factors)
        if not self.factors or any(not f > 0 for f in self.factors):
            raise ValueError("SpeedPerturb: factors must be positive, got %r" % (factors,))
        self.resamplers = {f: Resampler(int(round(self.sample_frequency * f)), self.sample_frequency, device) for f in self.factors}

    def __call__(self, waves, factor, lengths=None):
        """The batch perturbed by `factor`, one of self.factors: Resampler's call and return."""
        r = self.resamplers.get(float(factor))
        if r is None:
            raise ValueError("SpeedPerturb: factor %r is not one of %r" % (factor, self.factors))
        return r(waves, lengths)


class FrameContext(object):
    """Deltas, splice, skip and downsample pad of a base batch on the device (frontend.frame_context): the loader keys left_ctx, right_ctx,
    n_skip_frame, n_downsample under the names left, right, skip, n_downsample, plus Kaldi's add-deltas (delta_order 0: none).  Holds no
    device state: the batch's device is the call's.  Options outside the kernel's limits raise RuntimeError at the first out_dim / call."""

    def __init__(self, left=0, right=0, skip=1, n_downsample=1, delta_order=0, delta_window=2):
        self.left, self.right, self.skip, self.n_downsample = int(left), int(right), int(skip), int(n_downsample)
        self.delta_order, self.delta_window = int(delta_order), int(delta_window)

    @classmethod
    def from_opts(cls, opts):
        """From a driver's options object: the keys SpeechDataset reads."""
        return cls(opts.left_ctx, opts.right_ctx, opts.n_skip_frame, opts.n_downsample)

    def _kw(self):
        return dict(left=self.left, right=self.right, skip=self.skip, n_downsample=self.n_downsample, delta_order=self.delta_order,
                    delta_window=self.delta_window)

    def out_dim(self, feat_dim):
        """Columns of the output for base features of feat_dim columns: (left + 1 + right) * feat_dim * (delta_order + 1)."""
        frontend.frame_context_tile(feat_dim, **self._kw())                 # (the limits)
        return (self.left + 1 + self.right) * int(feat_dim) * (self.delta_order + 1)

    def out_frames(self, num_frames):
        """Rows of an utterance of num_frames base frames: kept frames, padded to a multiple of n_downsample."""
        return frontend.context_frames(num_frames, self.skip, self.n_downsample)

    def __call__(self, feats, frames):
        """feats (B, Tin_max, F) float32 on the device, frames (B) a list or a device tensor -- a front-end's return values as they are.
        Returns (out (B, Tout_max, out_dim(F)) float32: the model's input, out_frames (B) int32, fractions (B) float32: the loader's
        input_sizes) on the same device."""
        return frontend.frame_context(feats, frames, **self._kw())


class SpecAugment(object):
    """SpecAugment (Park et al., Interspeech 2019) of a base batch on the device (frontend.spec_augment): a time warp of up to warp_window frames,
    num_freq_masks masks of up to freq_width columns and num_time_masks masks of up to min(time_width, time_ratio * T) frames, set to `fill`.
    Utterance number i of the stream draws from (seed, i) alone: the object keeps the running index -- start_index, advanced by B at every
    call without utt_offset -- and no device state.  Everything is off by default; DEFAULTS is what the driver key `spec_augment: true`
    switches on: the paper's LD policy scaled to 81-column, three-second utterances.  Nobody has measured an error rate with it here."""

    DEFAULTS = dict(warp_window=5, num_freq_masks=2, freq_width=15, num_time_masks=2, time_width=40, time_ratio=0.2)

    def __init__(self, warp_window=0, num_freq_masks=0, freq_width=0, num_time_masks=0, time_width=0, time_ratio=1.0, fill=0.0, seed=0,
                 start_index=0):
        self.warp_window, self.num_freq_masks, self.freq_width = int(warp_window), int(num_freq_masks), int(freq_width)
        self.num_time_masks, self.time_width = int(num_time_masks), int(time_width)
        self.time_ratio, self.fill = float(time_ratio), float(fill)
        self.seed, self.index = int(seed), int(start_index)

    @classmethod
    def from_opts(cls, mapping, seed=0):
        """From the driver key's value: `True` for DEFAULTS, or a mapping of option names (the ones it leaves out stay off)."""
        if mapping is True:
            return cls(seed=seed, **cls.DEFAULTS)
        if not hasattr(mapping, "items"):
            raise ValueError("spec_augment: expected true or a mapping of %s, got %r" % (", ".join(frontend.SPEC_AUGMENT_OPTIONS), mapping))
        unknown = sorted(set(mapping) - set(frontend.SPEC_AUGMENT_OPTIONS))
        if unknown:
            raise ValueError("spec_augment: unknown option(s) %s (known: %s)" % (", ".join(unknown), ", ".join(frontend.SPEC_AUGMENT_OPTIONS)))
        return cls(seed=seed, **dict(mapping))

    def _kw(self):
        return {k: getattr(self, k) for k in frontend.SPEC_AUGMENT_OPTIONS}

    def plan(self, T, F, utt_index):
        """The warp and the masks of utterance utt_index with T frames of F columns (frontend.spec_augment_plan; no device)."""
        return frontend.spec_augment_plan(T, F, self.seed, utt_index, **self._kw())

    def __call__(self, feats, frames, utt_offset=None):
        """feats (B, Tmax, F) float32 on the device, frames (B) a list or a device tensor.  Utterance b is number utt_offset + b of the
        stream; without utt_offset, the running index, which then advances by B.  Returns the augmented batch, a new tensor."""
        out = frontend.spec_augment(feats, frames, self.seed, self.index if utt_offset is None else utt_offset, **self._kw())
        if utt_offset is None:
            self.index += int(feats.shape[0])
        return out


class Reverberate(object):
    """Multi-condition data on the waveform (frontend.reverberate; Kaldi's wav-reverberate): with probability rir_prob one room impulse response
    of the bank is convolved into an utterance, with probability noise_prob one noise of the bank is added at one of its SNRs, and
    normalize keeps the utterance's power.  `bank`: an frontend.ReverbBank, or (rirs, noises, sample_frequency[, snrs]) to build one from lists
    of 1-D arrays on the waveforms' scale.  Utterance number i of the stream draws from (seed, i) alone: the object keeps the running index
    -- start_index, advanced by B at every call without utt_offset -- as SpecAugment does.  The result is float32 on the input's scale:
    any front-end takes it as its waveform batch."""

    def __init__(self, bank, rir_prob=1.0, noise_prob=1.0, normalize=True, seed=0, device="cuda:0", start_index=0):
        self.device = torch.device(device)
        self.bank = bank if isinstance(bank, frontend.ReverbBank) else frontend.ReverbBank(*bank)
        self.rir_prob, self.noise_prob, self.normalize = float(rir_prob), float(noise_prob), bool(normalize)
        self.seed, self.index = int(seed), int(start_index)
        frontend.reverb_plan(self.bank, self.seed, 0, self.rir_prob, self.noise_prob)       # (the probabilities' limits, before any launch)

    def plan(self, utt_index):
        """The draws of utterance utt_index (frontend.reverb_plan; no device)."""
        return frontend.reverb_plan(self.bank, self.seed, utt_index, self.rir_prob, self.noise_prob)

    def __call__(self, waves, lengths=None, utt_offset=None):
        """waves as Fbank takes them: a list of 1-D waveforms, or a padded (B, Nmax) batch with `lengths`.  Utterance b is number
        utt_offset + b of the stream; without utt_offset, the running index, which then advances by B.  Returns (out (B, Nmax) float32
        zero-padded on the device, lengths): any front-end's (waves, lengths) form."""
        waves, lengths = _batch("Reverberate", waves, lengths)
        out = frontend.reverberate(waves.to(self.device), lengths, self.bank, self.seed, self.index if utt_offset is None else utt_offset,
                              rir_prob=self.rir_prob, noise_prob=self.noise_prob, normalize=self.normalize)
        if utt_offset is None:
            self.index += int(out.shape[0])
        return out, lengths


class GlobalCMVN(object):
    """One global mean / variance normalisation: Kaldi's CMVN statistics matrix, (2, F + 1) doubles -- row 0 the sums and the frame count,
    row 1 the sums of squares and 0 -- kept on `device`.  A CPU device serves loading, saving and mean_scale; accumulate needs the GPU."""

    def __init__(self, feat_dim, device="cpu"):
        self.feat_dim = int(feat_dim)
        self.stats = torch.zeros((2, self.feat_dim + 1), dtype=torch.float64, device=device)

    def accumulate(self, feats, frames):
        frontend.cmvn_accumulate(feats, frames, self.stats)
        return self

    def mean_scale(self, device=None):
        """(mean, scale) float32: mean = sum / n, var = max(sumsq / n - mean^2, 1e-20), scale = 1 / sqrt(var) (apply-cmvn --norm-vars=true),
        computed in double and rounded once.  numpy arrays, or tensors on `device`."""
        s = self.stats.cpu().numpy()
        n = s[0, -1]
        if not n > 0:
            raise ValueError("GlobalCMVN: no frames accumulated")
        mean = s[0, :-1] / n
        var = np.maximum(s[1, :-1] / n - mean * mean, 1e-20)
        mean, scale = mean.astype(np.float32), (1.0 / np.sqrt(var)).astype(np.float32)
        if device is None:
            return mean, scale
        return torch.from_numpy(mean).to(device), torch.from_numpy(scale).to(device)

    def save_kaldi_text(self, path):
        """The text form of `compute-cmvn-stats --binary=false`: ` [`, one indented row per line, `]`.  Values carry 17 significant digits
        (Kaldi's own writer keeps fewer; its reader takes either)."""
        s = self.stats.cpu().numpy()
        with open(path, "w") as f:
            f.write(" [")
            for row in s:
                f.write("\n  " + "".join("%.17g " % v for v in row))
            f.write("]\n")

    @classmethod
    def load_kaldi_text(cls, path, device="cpu"):
        """Reads save_kaldi_text's layout, and the same matrix behind an archive key (`global [ ...`)."""
        text = open(path).read()
        lo, hi = text.find("["), text.rfind("]")
        if lo < 0 or hi < lo:
            raise ValueError("%s: not a Kaldi text matrix" % path)
        rows = [[float(v) for v in line.split()] for line in text[lo + 1:hi].strip().splitlines() if line.strip()]
        if len(rows) != 2 or len(rows[0]) != len(rows[1]) or len(rows[0]) < 2:
            raise ValueError("%s: expected a 2 x (F + 1) CMVN statistics matrix" % path)
        out = cls(len(rows[0]) - 1, device)
        out.stats.copy_(torch.tensor(rows, dtype=torch.float64))
        return out


def read_utt2spk(path):
    """Kaldi's utt2spk file, one `<utterance> <speaker>` per line: {utterance: speaker}, in file order.  ValueError for a line with another
    number of fields or an utterance given twice."""
    out = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected '<utterance> <speaker>'" % (path, ln))
            if parts[0] in out:
                raise ValueError("%s:%d: utterance %s is given twice" % (path, ln, parts[0]))
            out[parts[0]] = parts[1]
    return out


class SpeakerCMVN(object):
    """Mean / variance normalisation per speaker: one Kaldi statistics matrix per name of `speakers`, (G, 2, F + 1) doubles kept on `device`
    -- compute-cmvn-stats --spk2utt and apply-cmvn --utt2spk.  With every utterance its own speaker it is per-utterance CMVN.  A CPU
    device serves loading and saving; accumulate and apply need the GPU.  Statistics are formed into mean and scale on the device by the
    apply call itself: nothing comes back to the host in between."""

    def __init__(self, feat_dim, speakers, device="cpu"):
        self.feat_dim = int(feat_dim)
        self.speakers = [str(s) for s in speakers]
        self.index = {s: g for g, s in enumerate(self.speakers)}
        if not self.speakers or len(self.index) != len(self.speakers):
            raise ValueError("SpeakerCMVN: expected at least one speaker and every name once")
        self.stats = torch.zeros((len(self.speakers), 2, self.feat_dim + 1), dtype=torch.float64, device=device)

    def _ids(self, speakers_of_batch):
        try:
            return [self.index[str(s)] for s in speakers_of_batch]
        except KeyError as e:
            raise ValueError("SpeakerCMVN: unknown speaker %s" % e)

    def accumulate(self, feats, frames, speakers_of_batch):
        frontend.cmvn_accumulate_groups(feats, frames, self._ids(speakers_of_batch), self.stats)
        return self

    def apply(self, feats, frames, speakers_of_batch, norm_vars=True, out=None):
        """feats (B, Tmax, F) normalised with the statistics of each utterance's speaker (apply-cmvn --norm-vars=<norm_vars>); rows at or
        beyond frames[b] come out as zeros.  A speaker without accumulated frames leaves its utterances as they are."""
        return frontend.cmvn_apply(feats, frames, self.stats, self._ids(speakers_of_batch), norm_vars=norm_vars, out=out)

    def save_kaldi_text(self, path):
        """The text archive of `compute-cmvn-stats --spk2utt=... ark,t:`: per speaker `<speaker>  [`, one indented row per line, `]`.  Values
        carry 17 significant digits, as GlobalCMVN's."""
        s = self.stats.cpu().numpy()
        with open(path, "w") as f:
            for name, mat in zip(self.speakers, s):
                f.write(name + "  [")
                for row in mat:
                    f.write("\n  " + "".join("%.17g " % v for v in row))
                f.write("]\n")

    @classmethod
    def load_kaldi_text(cls, path, device="cpu"):
        """Reads save_kaldi_text's layout (and Kaldi's own, which keeps fewer digits): speakers in file order."""
        names, mats, cur = [], [], None
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                parts = line.split()
                if not parts:
                    continue
                if cur is None:
                    if len(parts) < 2 or parts[1] != "[":
                        raise ValueError("%s:%d: expected '<speaker>  ['" % (path, ln))
                    names.append(parts[0])
                    cur, parts = [], parts[2:]
                    if not parts:
                        continue
                closed = parts[-1] == "]"
                if closed:
                    parts = parts[:-1]
                if parts:
                    cur.append([float(v) for v in parts])
                if closed:
                    if len(cur) != 2 or len(cur[0]) != len(cur[1]) or len(cur[0]) < 2 or (mats and len(cur[0]) != len(mats[0][0])):
                        raise ValueError("%s:%d: expected a 2 x (F + 1) CMVN statistics matrix for %s" % (path, ln, names[-1]))
                    mats.append(cur)
                    cur = None
        if cur is not None or not mats:
            raise ValueError("%s: not a Kaldi text archive of CMVN statistics" % path)
        out = cls(len(mats[0][0]) - 1, names, device)
        out.stats.copy_(torch.tensor(mats, dtype=torch.float64))
        return out


class SlidingCMVN(object):
    """Kaldi's apply-cmvn-sliding under its option names and defaults: every frame normalised by the mean (and, with normalize_variance,
    the variance) of a window of cmn_window frames around (center) or before it.  Called as (feats, frames) on a zero-padded device batch;
    returns a new (B, Tmax, F) tensor (frontend.cmvn_sliding)."""

    def __init__(self, cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False):
        self.cmn_window, self.min_cmn_window = int(cmn_window), int(min_cmn_window)
        self.normalize_variance, self.center = bool(normalize_variance), bool(center)
        if self.cmn_window < 1 or not 1 <= self.min_cmn_window <= self.cmn_window:
            raise ValueError("SlidingCMVN: cmn_window >= 1 and 1 <= min_cmn_window <= cmn_window needed, got %d and %d"
                             % (self.cmn_window, self.min_cmn_window))

    def __call__(self, feats, frames):
        return frontend.cmvn_sliding(feats, frames, cmn_window=self.cmn_window, min_cmn_window=self.min_cmn_window,
                                normalize_variance=self.normalize_variance, center=self.center)


def _riff(path, data):
    if data[8:12] != b"WAVE":
        raise NotImplementedError("%s: RIFF file of type %r, not WAVE" % (path, data[8:12]))
    pos, fmt = 12, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE and len(body) >= 26:                   # WAVE_FORMAT_EXTENSIBLE: the real tag opens the sub-format
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif tag == b"data":
            if fmt is None:
                raise ValueError("%s: data chunk before fmt chunk" % path)
            code, channels, rate, _, _, bits = fmt
            if code != 1 or bits != 16 or channels != 1:
                raise NotImplementedError("%s: WAVE format tag %d, %d bit, %d channel(s); only PCM (1), 16 bit, mono is read" % (path, code, bits, channels))
            return np.frombuffer(body[:len(body) // 2 * 2], dtype="<i2").astype(np.int16), rate
        pos += 8 + size + (size & 1)
    raise ValueError("%s: no data chunk" % path)


def _sphere(path, data):
    try:
        head_bytes = int(data[8:16].split()[0])
    except (ValueError, IndexError):
        raise ValueError("%s: malformed SPHERE header" % path)
    fields = {}
    for line in data[16:head_bytes].decode("latin-1").splitlines():
        parts = line.split(None, 2)
        if parts and parts[0] == "end_head":
            break
        if len(parts) == 3:
            fields[parts[0]] = parts[2].strip()
    coding = fields.get("sample_coding", "pcm")
    channels, nbytes = int(fields.get("channel_count", 1)), int(fields.get("sample_n_bytes", 2))
    if coding != "pcm" or channels != 1 or nbytes != 2:
        raise NotImplementedError("%s: SPHERE sample_coding %r, %d byte(s) per sample, %d channel(s); only uncompressed pcm, 2 bytes, mono is read"
                                  % (path, coding, nbytes, channels))
    order = fields.get("sample_byte_format", "01")
    if order not in ("01", "10"):
        raise NotImplementedError("%s: SPHERE sample_byte_format %r" % (path, order))
    body = data[head_bytes:]
    if "sample_count" in fields:
        body = body[:2 * int(fields["sample_count"])]
    return np.frombuffer(body[:len(body) // 2 * 2], dtype="<i2" if order == "01" else ">i2").astype(np.int16), int(fields["sample_rate"])


def read_wave(path):
    """(int16 samples, sample rate) of a RIFF WAVE file (PCM, 16 bit, mono) or an uncompressed NIST SPHERE file such as TIMIT's (the 1024-byte
    text header, sample_coding pcm, 2 bytes per sample, either byte order, one channel).  Anything else raises NotImplementedError naming
    what the file holds."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] == b"RIFF":
        return _riff(path, data)
    if data[:7] == b"NIST_1A":
        return _sphere(path, data)
    raise NotImplementedError("%s: neither a RIFF nor a NIST SPHERE file (starts with %r)" % (path, data[:8]))
