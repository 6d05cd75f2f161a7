"""The device feature front-end over the C ABI of libctcn.so: waveform -> features -> the batch the model consumes.

Filterbank, MFCC and the two spectrograms, resampling, reverberation and noise, SpecAugment, deltas / splice / skip, three kinds of CMVN and
pitch.  Every device entry point enqueues hand-written gfx950 kernels on torch's current HIP stream and takes device tensors only (no CPU
fallback); the `*_frames`, `*_plan`, `*_host` functions and the plan objects are host arithmetic.  No autograd anywhere in this module.
ops.py re-exports the public names; what the wrappers share -- the two batch checks, the plan base class, the options-to-struct
conversion, the pointer and return-code helpers -- is defined once, right below.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import _need_gpu, _ptr

_U64 = (1 << 64) - 1                    # seeds and running indices go to the library modulo 2^64


# --------------------------------------------------------------------------------------------------
# what the wrappers share
# --------------------------------------------------------------------------------------------------
def _np_ptr(a, when=True):
    """The data pointer of a numpy array for the C ABI; None where `when` is false (an empty array: the library takes NULL)."""
    return a.ctypes.data_as(ctypes.c_void_p) if when else None


def _checked(r, what):
    """r, a count or size from the library, after raising (RuntimeError, the library's message) for a negative one."""
    if r < 0:
        _lib.check(r, what)
    return r


_CONVERT = {bool: lambda v: int(bool(v)), float: float, int: int}


class _StructFrom(object):
    """The one way from options to an option struct of the C ABI.  `defaults` names the struct's fields in their order; every value is
    converted by the type of its default (bool to 0 / 1, float, int).  `error`: what an unknown keyword option raises."""

    def __init__(self, struct, defaults, error=ValueError):
        assert [k for k, _ in struct._fields_] == list(defaults), struct
        self.struct, self.defaults, self.error = struct, defaults, error
        self._convert = [_CONVERT[type(d)] for d in defaults.values()]

    def __call__(self, *values):
        """The struct of one value per option, in the defaults' order."""
        return self.struct(*[c(v) for c, v in zip(self._convert, values)])

    def keywords(self, who, kw):
        """The struct of the defaults overridden by the keyword options `kw`."""
        merged = {**self.defaults, **kw}
        if len(merged) != len(self.defaults):
            raise self.error("ctc_pytorch_amd.%s: unknown option(s) %s (known: %s)" % (who, ", ".join(sorted(set(kw) - set(self.defaults))),
                                                                                     ", ".join(self.defaults)))
        return self(*merged.values())


def _expect(who, obj, cls):
    if not isinstance(obj, cls):
        raise TypeError("ctc_pytorch_amd.%s: expected a %s, got %s" % (who, cls.__name__, type(obj).__name__))


def _int32_on(values, device):
    """Counts as an int32 tensor on `device`: a tensor is converted where it lives (nothing is read back), a host sequence is uploaded."""
    if torch.is_tensor(values):
        return values.to(device=device, dtype=torch.int32).contiguous()
    return torch.as_tensor([int(v) for v in values], dtype=torch.int32).to(device)


def _wave_batch(who, wave, lengths, size=None, also=()):
    """The check every waveform entry point makes -- rank 2, on the device (with the tensors of `also`), float32 or int16, one length per
    utterance and at least one utterance.  Returns (contiguous wave, lengths as an int32 device tensor, sizes).  `size` is the caller's
    host rule from an utterance's samples to what sizes its output (its frames, its resampled samples): with it the lengths are read on
    the host, sizes = [size(n clamped to [0, Nmax])], and the lengths are uploaded as given AFTER that arithmetic -- the upload waits for
    the stream, what the host does in front of it runs beside the kernels already queued.  Without it a device tensor of lengths is taken
    as it is, nothing is read back and sizes is None."""
    if wave.dim() != 2:
        raise ValueError("ctc_pytorch_amd.%s: expected wave (B, Nmax), got %s" % (who, tuple(wave.shape)))
    _need_gpu(wave, *also)
    if wave.dtype not in (torch.float32, torch.int16):
        raise TypeError("ctc_pytorch_amd.%s: expected float32 or int16 samples, got %s" % (who, wave.dtype))
    B, Nmax = wave.shape

    def counted(n):
        if n != B or B == 0:
            raise ValueError("ctc_pytorch_amd.%s: %d lengths for a batch of %d" % (who, n, B))

    if size is None:
        lens, sizes = _int32_on(lengths, wave.device), None
        counted(lens.numel())
    else:
        host = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        counted(len(host))
        sizes = [size(min(max(n, 0), Nmax)) for n in host]
        lens = torch.as_tensor(host, dtype=torch.int32).to(wave.device)
    return wave.contiguous(), lens, sizes


def _feature_batch(who, feats, frames, dtype_error=TypeError, refuse_empty=False):
    """The check every feature entry point makes -- a rank-3 float32 tensor on the device, one frame count per utterance.  Returns the frame
    counts as an int32 device tensor (a device tensor is taken as it is, nothing is read back).  dtype_error: what a dtype other than
    float32 raises; as ValueError it is part of the shape check, in front of the device check.  refuse_empty: B == 0 or F == 0 raises
    (callers that return early for an empty batch leave it off)."""
    is_tensor = torch.is_tensor(feats)
    wrong_dtype = is_tensor and feats.dtype != torch.float32
    if not is_tensor or feats.dim() != 3 or (wrong_dtype and dtype_error is ValueError):
        raise ValueError("ctc_pytorch_amd.%s: expected feats (B, Tmax, F) float32, got %s" % (
            who, "%s %s" % (tuple(feats.shape), feats.dtype) if is_tensor else type(feats).__name__))
    _need_gpu(feats, frames if torch.is_tensor(frames) else None)
    if wrong_dtype:
        raise dtype_error("ctc_pytorch_amd.%s: expected float32 features, got %s" % (who, feats.dtype))
    frames = _int32_on(frames, feats.device)
    B, _, F = feats.shape
    if frames.numel() != B or (refuse_empty and (B == 0 or F == 0)):
        raise ValueError("ctc_pytorch_amd.%s: %d frame counts for a batch of %s" % (who, frames.numel(), tuple(feats.shape)))
    return frames


class _DeviceBlock(object):
    """A block of uint32 words built on the host (`host`, layout in include/ctcn.h) and uploaded once per device, on first use."""
    _upload = np.int32                                                  # the view that is uploaded (PitchPlan: int64, its block holds doubles)

    def _keep(self, host):
        self.host, self._dev = host, {}

    def on(self, device):
        """The block in the memory of `device`, uploaded on first use."""
        key = (device.type, device.index)
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.host.view(self._upload)).to(device)
        return t

    def _host_ptr(self):
        return _np_ptr(self.host)


class _Plan(_DeviceBlock):
    """A block the library sizes and fills from one option struct: ctcn_<_name>_plan_bytes, then ctcn_<_name>_plan -- a RuntimeError there,
    when the object is made and before any launch, for a configuration the kernel does not take.  The allocation is aligned to the
    uploaded view's word and holds at least _min_words of them."""
    _name = None
    _min_words = 1

    def _build(self, opts):
        L = _lib.lib()
        self.opts = opts
        nbytes = getattr(L, "ctcn_%s_plan_bytes" % self._name)(ctypes.byref(opts))
        word = np.dtype(self._upload).itemsize
        buf = np.zeros(max(nbytes // word, self._min_words), dtype="u%d" % word).view(np.uint32)
        _lib.check(getattr(L, "ctcn_%s_plan" % self._name)(ctypes.byref(opts), _np_ptr(buf), nbytes), "%s_plan" % self._name)
        self._keep(buf)
        return buf


# --------------------------------------------------------------------------------------------------
# filterbank front-end (fbank.hip): waveform -> normalised log-mel features (the global CMVN statistics, cmvn.hip: cmvn_accumulate below)
# --------------------------------------------------------------------------------------------------
def fbank_frames(num_samples, frame_length, frame_shift, snip_edges=True):
    """Frames of a signal of num_samples samples (ctcn_fbank_frames; lengths in samples): Kaldi's two rules.  Host arithmetic, no device."""
    r = _lib.lib().ctcn_fbank_frames(int(num_samples), int(frame_length), int(frame_shift), int(bool(snip_edges)))
    if r < 0:
        raise ValueError("ctc_pytorch_amd.fbank_frames: bad arguments (samples %r, frame length %r, shift %r)" % (num_samples, frame_length, frame_shift))
    return r


class FbankPlan(_Plan):
    """The plan of one filterbank configuration (ctcn_fbank_plan: window, twiddles, mel filters): built on the host from an _lib.FbankOpts when
    the object is made -- a RuntimeError here, before any launch, for a configuration the kernel does not take -- and uploaded once per
    device on first use.  `host` is the block as uint32 words (layout in include/ctcn.h)."""
    _name = "fbank"                                                    # ctcn_<name>_plan_bytes, ctcn_<name>_plan, ctcn_<name>

    def __init__(self, opts):
        self._build(opts)
        self.frame_length = int(float(opts.samp_freq) * 0.001 * float(opts.frame_length_ms))
        self.frame_shift = int(float(opts.samp_freq) * 0.001 * float(opts.frame_shift_ms))
        self.padded_length = 1 << (self.frame_length - 1).bit_length()
        self.num_mel_bins = int(getattr(opts, "num_mel_bins", 0))      # (the spectrogram has no mel bank)
        self.feat_dim = self._feat_dim(opts)
        self.snip_edges = bool(opts.snip_edges)

    def _feat_dim(self, opts):
        return int(opts.num_mel_bins) + (1 if opts.use_energy else 0)

    def num_frames(self, num_samples):
        return fbank_frames(num_samples, self.frame_length, self.frame_shift, self.snip_edges)


class MfccPlan(FbankPlan):
    """The plan of one MFCC configuration (ctcn_mfcc_plan, from an _lib.MfccOpts): the filterbank plan of the same frame and mel options,
    then the DCT table (bin-major) and the lifter.  feat_dim = num_ceps."""
    _name = "mfcc"

    def _feat_dim(self, opts):
        self.num_ceps = int(opts.num_ceps)
        return self.num_ceps


class SpectrogramPlan(FbankPlan):
    """The plan of one spectrogram configuration (ctcn_spectrogram_plan, from an _lib.SpectrogramOpts): the window and the twiddles of the
    filterbank plan of the same frame options.  feat_dim = padded_length / 2 + 1; there is no mel bank (num_mel_bins is 0)."""
    _name = "spectrogram"

    def _feat_dim(self, opts):
        return self.padded_length // 2 + 1


def _frontend(name, wave, lengths, plan, mean, scale, dither, seed, utt_offset):
    """The body of fbank, mfcc and spectrogram: validation, output allocation, ctcn_<name>."""
    wave, lens, counts = _wave_batch(name, wave, lengths, plan.num_frames, also=(mean, scale))
    if (mean is None) != (scale is None):
        raise ValueError("ctc_pytorch_amd.%s: mean and scale come together" % name)
    if not float(dither) >= 0.0:
        raise ValueError("ctc_pytorch_amd.%s: dither must not be negative, got %r" % (name, dither))
    (B, Nmax), dev, F = wave.shape, wave.device, plan.feat_dim
    for v in (mean, scale):
        if v is not None and (v.dtype != torch.float32 or v.numel() != F):
            raise ValueError("ctc_pytorch_amd.%s: mean / scale must hold %d float32 values" % (name, F))
    mean, scale = (None, None) if mean is None else (mean.contiguous(), scale.contiguous())
    Tmax = max(counts)
    feats = torch.empty((B, Tmax, F), dtype=torch.float32, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    entry = getattr(_lib.lib(), "ctcn_" + name)
    _lib.check(entry(_ptr(wave), int(wave.dtype == torch.int16), _ptr(lens), ctypes.byref(plan.opts), _ptr(plan.on(dev)), _ptr(mean), _ptr(scale),
                     _ptr(feats) if Tmax else None, _ptr(frames), B, Nmax, Tmax, float(dither), int(seed) & _U64, int(utt_offset),
                     _lib.stream_ptr()), name)
    return feats, frames


def fbank(wave, lengths, plan, mean=None, scale=None, dither=0.0, seed=0, utt_offset=0):
    """Filterbank features of a padded batch of waveforms (ctcn_fbank; the computation, step by step, in include/ctcn.h): wave (B, Nmax)
    float32 on Kaldi's scale (the int16 range) or int16; lengths (B) samples, a list or a tensor (read on the host: the frame counts size
    the output); plan a FbankPlan; mean / scale (F) float32 device vectors or None: (x - mean) * scale applied by the same kernel.
    Returns (feats (B, Tmax, F) float32, frames (B) int32) with Tmax = the largest frame count; rows from frames[b] on are zero.  dither > 0
    adds dither * N(0, 1) per extracted sample, a function of (seed, b + utt_offset, frame, sample) alone.  No autograd; device tensors only
    (no CPU fallback)."""
    if type(plan) is not FbankPlan:                                     # (MfccPlan and SpectrogramPlan carry other option structs)
        raise TypeError("ctc_pytorch_amd.fbank: expected a FbankPlan, got %s" % type(plan).__name__)
    return _frontend("fbank", wave, lengths, plan, mean, scale, dither, seed, utt_offset)


def mfcc(wave, lengths, plan, mean=None, scale=None, dither=0.0, seed=0, utt_offset=0):
    """MFCCs of a padded batch of waveforms (ctcn_mfcc: the filterbank kernel with the DCT, the lifter and Kaldi's column rules behind its
    log-mel stage; include/ctcn.h).  The contract of fbank with plan a MfccPlan and F = num_ceps."""
    _expect("mfcc", plan, MfccPlan)
    return _frontend("mfcc", wave, lengths, plan, mean, scale, dither, seed, utt_offset)


def spectrogram(wave, lengths, plan, mean=None, scale=None, dither=0.0, seed=0, utt_offset=0):
    """Kaldi's spectrogram features of a padded batch of waveforms (ctcn_spectrogram: the filterbank kernel without the mel bank -- the log
    power of bins 0 .. Npad / 2 with the log energy in column 0; include/ctcn.h).  The contract of fbank with plan a SpectrogramPlan and
    F = Npad / 2 + 1."""
    _expect("spectrogram", plan, SpectrogramPlan)
    return _frontend("spectrogram", wave, lengths, plan, mean, scale, dither, seed, utt_offset)


class LogSpecPlan(_Plan):
    """The plan of one configuration of the recipe's log-magnitude STFT (ctcn_logspec_plan, from an _lib.LogSpecOpts: symmetric window,
    twiddles): built on the host when the object is made -- a RuntimeError here, before any launch, for a configuration the kernel does not
    take (n_fft other than 256, 400, 512, 1024) -- and uploaded once per device on first use.  `host`: the block as uint32 words."""
    _name = "logspec"

    def __init__(self, opts):
        self._build(opts)
        self.n_fft = int(float(opts.sample_rate) * float(opts.window_size))
        self.hop = int(float(opts.sample_rate) * float(opts.window_stride))
        self.feat_dim = self.n_fft // 2 + 1
        self.normalize = bool(opts.normalize)

    def num_frames(self, num_samples):
        r = _lib.lib().ctcn_logspec_frames(int(num_samples), self.hop)
        if r < 0:
            raise ValueError("ctc_pytorch_amd.LogSpecPlan.num_frames: bad sample count %r" % (num_samples,))
        return r


def log_spectrum(wave, lengths, plan):
    """The recipe's spectrogram (make_spectrum.py: centred STFT over the reflected signal, symmetric window, log1p of the magnitude, one mean
    and standard deviation per utterance; ctcn_logspec, step by step in include/ctcn.h) of a padded batch: wave (B, Nmax) float32 or int16,
    lengths (B) samples (read on the host), plan a LogSpecPlan.  Returns (feats (B, Tmax, n_fft / 2 + 1) float32 with rows from frames[b] on
    zero, frames (B) int32, stats (B, 2) float32: the mean and standard deviation applied -- or, with normalize off, that would have been).
    No autograd; device tensors only (no CPU fallback)."""
    _expect("log_spectrum", plan, LogSpecPlan)
    wave, lens, counts = _wave_batch("log_spectrum", wave, lengths, plan.num_frames)
    (B, Nmax), dev = wave.shape, wave.device
    Tmax = max(counts)
    feats = torch.empty((B, Tmax, plan.feat_dim), dtype=torch.float32, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    stats = torch.empty((B, 2), dtype=torch.float32, device=dev)
    need = _lib.lib().ctcn_logspec_ws_bytes(ctypes.byref(plan.opts), B, Tmax)
    ws = _lib.workspace(dev, nbytes=need, tag="logspec")
    _lib.check(_lib.lib().ctcn_logspec(_ptr(wave), int(wave.dtype == torch.int16), _ptr(lens), ctypes.byref(plan.opts), _ptr(plan.on(dev)),
                                       _ptr(feats) if Tmax else None, _ptr(frames), _ptr(stats), B, Nmax, Tmax, _ptr(ws), ws.numel(),
                                       _lib.stream_ptr()), "logspec")
    return feats, frames, stats


# resampling in front of the feature kernels (resample.hip): another sample rate, speed perturbation
def resample_samples(num_samples, orig_freq, new_freq):
    """Samples a signal of num_samples samples has after resampling from orig_freq to new_freq Hz (ctcn_resample_samples: ceil(n new / orig),
    Kaldi's count with flush).  Host arithmetic, no device.  ValueError for bad arguments, RuntimeError for a length beyond int32."""
    r = _lib.lib().ctcn_resample_samples(int(num_samples), int(orig_freq), int(new_freq))
    if r == -3:
        _lib.check(r, "resample_samples")
    if r < 0:
        raise ValueError("ctc_pytorch_amd.resample_samples: bad arguments (samples %r, rates %r -> %r)" % (num_samples, orig_freq, new_freq))
    return r


class ResamplePlan(_Plan):
    """The plan of one pair of rates (ctcn_resample_plan: Kaldi's LinearResample filter, one row of float32 weights per output phase): built on
    the host when the object is made -- a RuntimeError here, before any launch, for what the kernel does not take (a table beyond its LDS
    budget, a cutoff above the lower Nyquist frequency, num_zeros or a rate that is not positive) -- and uploaded once per device on first
    use.  cutoff (Hz) defaults to Kaldi's 0.99 * 0.5 * min(rates).  `host` is the block as uint32 words (layout in include/ctcn.h); `first`,
    `ntaps` (ou) and `weights` (ou, row stride) are numpy views of it: the table the kernel reads.  `tile`: outputs per workgroup."""
    _name = "resample"
    _min_words = 8                                                     # (the header, read below whatever the library filled)

    def __init__(self, orig_freq, new_freq, num_zeros=6, cutoff=None):
        if cutoff is None:
            cutoff = 0.99 * 0.5 * min(int(orig_freq), int(new_freq))
        buf = self._build(_lib.ResampleOpts(cutoff=float(cutoff), orig_freq=int(orig_freq), new_freq=int(new_freq), num_zeros=int(num_zeros)))
        self.orig_freq, self.new_freq, self.num_zeros, self.cutoff = int(orig_freq), int(new_freq), int(num_zeros), float(cutoff)
        hdr = buf[:8].view(np.int32)
        self.ou, self.iu, self.stride, self.max_taps, self.tile = (int(v) for v in hdr[:5])
        self.first = buf[8:8 + self.ou].view(np.int32)
        self.ntaps = buf[8 + self.ou:8 + 2 * self.ou].view(np.int32)
        self.weights = buf[8 + 2 * self.ou:8 + 2 * self.ou + self.ou * self.stride].view(np.float32).reshape(self.ou, self.stride)

    def num_samples(self, num_samples):
        return resample_samples(num_samples, self.orig_freq, self.new_freq)


def resample(wave, lengths, plan):
    """A padded batch of waveforms at plan.new_freq (ctcn_resample; the computation, step by step, in include/ctcn.h): wave (B, Nmax) float32
    or int16 at plan.orig_freq, lengths (B) samples, a list or a tensor (read on the host: the output lengths are host arithmetic), plan a
    ResamplePlan.  Returns (out (B, Mmax) float32 on the input's scale with zeros from the utterance's length on, out_lengths list of ints),
    Mmax the largest output length.  No autograd; device tensors only (no CPU fallback)."""
    _expect("resample", plan, ResamplePlan)
    wave, lens, out_lens = _wave_batch("resample", wave, lengths, plan.num_samples)
    (B, Nmax), dev = wave.shape, wave.device
    Mmax = max(out_lens)
    out = torch.empty((B, Mmax), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_resample(_ptr(wave), int(wave.dtype == torch.int16), _ptr(lens), ctypes.byref(plan.opts), _ptr(plan.on(dev)),
                                        _ptr(out) if Mmax else None, B, Nmax, Mmax, _lib.stream_ptr()), "resample")
    return out, out_lens


# deltas, splice, skip and the downsample pad behind the feature kernels (context.hip): base features -> the batch the model consumes
CONTEXT_OPTIONS = dict(left=0, right=0, skip=1, n_downsample=1, delta_order=0, delta_window=2)
_context_opts = _StructFrom(_lib.ContextOpts, CONTEXT_OPTIONS)


def context_frames(num_frames, skip=1, n_downsample=1):
    """Rows an utterance of num_frames frames has after frame skipping and the pad to a multiple of n_downsample (ctcn_context_frames:
    ceil(T / skip) rounded up; skip 0 and 1 keep every frame).  Host arithmetic, no device.  ValueError for bad arguments."""
    r = _lib.lib().ctcn_context_frames(int(num_frames), int(skip), int(n_downsample))
    if r < 0:
        raise ValueError("ctc_pytorch_amd.context_frames: bad arguments (frames %r, skip %r, n_downsample %r)" % (num_frames, skip, n_downsample))
    return r


def delta_scales(order, window=2):
    """Kaldi's delta filter of one order (ctcn_delta_scales): 2 * order * window + 1 float32 values, built on the host as DeltaFeatures builds
    them.  No device."""
    buf = np.zeros(2 * max(int(order), 0) * max(int(window), 0) + 1, dtype=np.float32)
    _checked(_lib.lib().ctcn_delta_scales(int(order), int(window), _np_ptr(buf)), "delta_scales")
    return buf


def frame_context_tile(feat_dim, left=0, right=0, skip=1, n_downsample=1, delta_order=0, delta_window=2):
    """Output rows one workgroup of frame_context writes under these options (ctcn_frame_context_tile).  RuntimeError for options outside the
    kernel's limits.  No device."""
    opts = _context_opts(left, right, skip, n_downsample, delta_order, delta_window)
    return _checked(_lib.lib().ctcn_frame_context_tile(ctypes.byref(opts), int(feat_dim)), "frame_context_tile")


def frame_context(feats, frames, left=0, right=0, skip=1, n_downsample=1, delta_order=0, delta_window=2):
    """Deltas, frame splicing, frame skipping and the downsample pad of a zero-padded base batch in one launch (ctcn_frame_context; the
    computation, step by step, in include/ctcn.h): feats (B, Tin_max, F) float32, frames (B) the utterances' frame counts -- a list or a
    device tensor (what Fbank returns), clamped to [0, Tin_max]; rows at or beyond them are never read.  Returns (out (B, Tout_max, F2)
    float32, out_frames (B) int32, fractions (B) float32 = out_frames / Tout_max as the host collate stores them) on the device, with
    F2 = (left + 1 + right) * F * (delta_order + 1) and Tout_max = context_frames(Tin_max, skip, n_downsample): sized from the input's
    shape, nothing is read back from the device.  No autograd; device tensors only (no CPU fallback)."""
    frames = _feature_batch("frame_context", feats, frames, refuse_empty=True)
    (B, Tin_max, F), dev = feats.shape, feats.device
    opts = _context_opts(left, right, skip, n_downsample, delta_order, delta_window)
    _lib.check(min(_lib.lib().ctcn_frame_context_tile(ctypes.byref(opts), F), 0), "frame_context")     # the limits, before anything is allocated
    Tout_max = context_frames(Tin_max, skip, n_downsample)
    feats = feats.contiguous()
    out = torch.empty((B, Tout_max, (opts.left + 1 + opts.right) * F * (opts.delta_order + 1)), dtype=torch.float32, device=dev)
    out_frames = torch.empty(B, dtype=torch.int32, device=dev)
    fractions = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_frame_context(_ptr(feats) if Tin_max else None, _ptr(frames), ctypes.byref(opts), _ptr(out) if Tout_max else None,
                                             _ptr(out_frames), _ptr(fractions), B, Tin_max, F, Tout_max, _lib.stream_ptr()), "frame_context")
    return out, out_frames, fractions


# SpecAugment on the base features, in front of frame_context (specaug.hip): time warp, frequency masks, time masks
_SPEC_AUGMENT_DEFAULTS = dict(warp_window=0, num_freq_masks=0, freq_width=0, num_time_masks=0, time_width=0, time_ratio=1.0, fill=0.0)
SPEC_AUGMENT_OPTIONS = tuple(_SPEC_AUGMENT_DEFAULTS)
_specaug_opts = _StructFrom(_lib.SpecAugOpts, _SPEC_AUGMENT_DEFAULTS, error=TypeError)      # (an unknown keyword raises what a call would)


def spec_augment_plan(T, F, seed, utt_index, **opts):
    """The intervals spec_augment uses for the utterance `utt_index` of T frames and F columns under `seed` (ctcn_spec_augment_plan):
    {"warp": (c, w) or None, "freq": [(f0, len), ...], "time": [(t0, len), ...]}.  Host arithmetic, no device.  RuntimeError for options
    outside the limits of include/ctcn.h."""
    o = _specaug_opts.keywords("spec_augment_plan", opts)
    warp = (ctypes.c_int32 * 2)()
    freq = (ctypes.c_int32 * (2 * max(o.num_freq_masks, 1)))()
    time = (ctypes.c_int32 * (2 * max(o.num_time_masks, 1)))()
    _lib.check(_lib.lib().ctcn_spec_augment_plan(ctypes.byref(o), int(seed) & _U64, int(utt_index) & _U64, int(T), int(F), warp, freq, time),
               "spec_augment_plan")
    return {"warp": (warp[0], warp[1]) if warp[1] > 0 else None,
            "freq": [(freq[2 * k], freq[2 * k + 1]) for k in range(o.num_freq_masks)],
            "time": [(time[2 * k], time[2 * k + 1]) for k in range(o.num_time_masks)]}


def spec_augment_host(feats_np, seed, utt_index, **opts):
    """spec_augment for ONE utterance on the host (ctcn_spec_augment_host: the interval and interpolation code the kernel is compiled
    from): feats_np (T, F) float32 numpy -> a new (T, F) float32 array.  No device."""
    x = np.ascontiguousarray(feats_np, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("ctc_pytorch_amd.spec_augment_host: expected feats (T, F), got %s" % (x.shape,))
    T, F = x.shape
    o = _specaug_opts.keywords("spec_augment_host", opts)
    out = np.empty_like(x)
    _lib.check(_lib.lib().ctcn_spec_augment_host(_np_ptr(x, T), T, F, ctypes.byref(o), int(seed) & _U64, int(utt_index) & _U64, _np_ptr(out, T)),
               "spec_augment_host")
    return out


def spec_augment(feats, frames, seed, utt_offset=0, **opts):
    """SpecAugment of a zero-padded base batch in one launch (ctcn_spec_augment; the computation, step by step, in include/ctcn.h): feats
    (B, Tmax, F) float32, frames (B) the utterances' frame counts -- a list or a device tensor, clamped to [0, Tmax]; rows at or beyond
    them are never read and come out as zeros.  Utterance b draws its warp and masks from (seed, utt_offset + b) alone.  Options:
    warp_window, num_freq_masks, freq_width, num_time_masks, time_width, time_ratio, fill (all off by default: the identity on the
    utterances' rows).  Returns out (B, Tmax, F) float32, a new tensor.  No autograd; device tensors only (no CPU fallback)."""
    frames = _feature_batch("spec_augment", feats, frames, refuse_empty=True)
    B, Tmax, F = feats.shape
    o = _specaug_opts.keywords("spec_augment", opts)
    feats = feats.contiguous()
    out = torch.empty((B, Tmax, F), dtype=torch.float32, device=feats.device)
    _lib.check(_lib.lib().ctcn_spec_augment(_ptr(feats) if Tmax else None, _ptr(frames), ctypes.byref(o), int(seed) & _U64, int(utt_offset) & _U64,
                                            _ptr(out) if Tmax else None, B, Tmax, F, _lib.stream_ptr()), "spec_augment")
    return out


# reverberation and additive noise on the waveform (reverb.hip): multi-condition data in front of the feature kernels
REVERB_LIMIT_FIELDS = ("tile", "tap_chunk", "power_chunk", "max_taps", "max_snrs", "run")
REVERB_OPTIONS = dict(rir_prob=1.0, noise_prob=1.0, normalize=True)
_reverb_opts = _StructFrom(_lib.ReverbOpts, REVERB_OPTIONS)


def reverb_limits():
    """The constants of reverb.hip (ctcn_reverb_limits): outputs per tile, taps per staged chunk, elements per power-sum chunk, the longest
    impulse response, the most SNRs, outputs per lane.  No device."""
    buf = (ctypes.c_int32 * len(REVERB_LIMIT_FIELDS))()
    _lib.check(_lib.lib().ctcn_reverb_limits(buf), "reverb_limits")
    return dict(zip(REVERB_LIMIT_FIELDS, (int(v) for v in buf)))


def _rows(who, what, arrays):
    """A list of 1-D arrays as (padded (rows, stride) float32, lengths int32); int16 rows are converted exactly."""
    rows = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    if any(r.ndim != 1 for r in rows):
        raise ValueError("ctc_pytorch_amd.%s: every %s must be a 1-D array" % (who, what))
    lens = np.asarray([r.shape[0] for r in rows], dtype=np.int32)
    out = np.zeros((len(rows), max([1] + [int(v) for v in lens])), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out, lens


class ReverbBank(_DeviceBlock):
    """The bank reverberate draws from (ctcn_reverb_bank): `rirs` and `noises`, lists of 1-D arrays (float32, or int16 converted exactly) on
    the scale of the waveforms they will meet, `snrs` the SNRs in dB a noise is added at (at most 16).  Either list may be empty.  Built on
    the host when the object is made -- the noise powers P_m, every impulse response's peak and early window, G_j = 10^(-snr_j / 10) -- with
    a RuntimeError here, before any launch, for what the kernel does not take (an empty row, an impulse response beyond `reverb_limits()
    ["max_taps"]`, more than 16 SNRs, a value that is not finite); uploaded once per device, at once when `device` is given.  `host` is the
    block as uint32 words (layout in include/ctcn.h); `rir_meta` (R, 4) = (K, peak, lo, hi), `noise_len` (N), `noise_power` (N), `snr_gain`
    (J) are numpy views of it."""

    def __init__(self, rirs, noises, sample_frequency, snrs=(20, 15, 10, 5, 0), device=None):
        L = _lib.lib()
        h, hl = _rows("ReverbBank", "impulse response", rirs)
        q, ql = _rows("ReverbBank", "noise", noises)
        R, N = self.R, self.N = len(hl), len(ql)
        self.snrs = np.asarray([float(v) for v in snrs], dtype=np.float64)
        J = self.J = int(self.snrs.shape[0]) if N else 0
        self.sample_frequency = float(sample_frequency)
        nbytes = L.ctcn_reverb_bank_bytes(R, h.shape[1] if R else 0, N, q.shape[1] if N else 0, J)
        buf = np.zeros(max(nbytes // 4, 16), dtype=np.uint32)
        _lib.check(L.ctcn_reverb_bank(_np_ptr(h, R), _np_ptr(hl, R), R, h.shape[1] if R else 0, _np_ptr(q, N), _np_ptr(ql, N), N,
                                      q.shape[1] if N else 0, _np_ptr(self.snrs, J), J, self.sample_frequency, _np_ptr(buf), nbytes), "reverb_bank")
        self._keep(buf)
        w = buf.view(np.int32)
        self.rir_stride, self.noise_stride, self.max_early = int(w[4]), int(w[5]), int(w[6])
        self.rir_meta = w[w[8]:w[8] + 4 * R].reshape(R, 4)
        self.noise_len = w[w[9]:w[9] + N]
        dbl = buf[w[10]:w[10] + 2 * (N + 16)].view(np.float64)
        self.noise_power, self.snr_gain = dbl[:N], dbl[N:N + J]
        if device is not None:
            self.on(torch.device(device))


def reverb_plan(bank, seed, utt_index, rir_prob=1.0, noise_prob=1.0):
    """The draws reverberate makes for utterance `utt_index` under `seed` (ctcn_reverb_plan): {"rir": r or None, "noise": m or None,
    "snr": the index into bank.snrs or None, "offset": the first noise sample or None}.  Host arithmetic, no device."""
    _expect("reverb_plan", bank, ReverbBank)
    o = _reverb_opts(rir_prob, noise_prob, True)
    d = (ctypes.c_int32 * 4)()
    _lib.check(_lib.lib().ctcn_reverb_plan(bank._host_ptr(), ctypes.byref(o), int(seed) & _U64, int(utt_index) & _U64, d), "reverb_plan")
    noise = d[1] >= 0
    return {"rir": int(d[0]) if d[0] >= 0 else None, "noise": int(d[1]) if noise else None, "snr": int(d[2]) if noise else None,
            "offset": int(d[3]) if noise else None}


def reverberate_host(wave_np, bank, seed, utt_index, rir_prob=1.0, noise_prob=1.0, normalize=True):
    """reverberate for ONE utterance on the host (ctcn_reverb_host: the draw, gain, mix and scale code the kernels are compiled from):
    wave_np (n) int16 or float32 numpy -> a new (n) float32 array.  No device."""
    _expect("reverberate_host", bank, ReverbBank)
    x = np.ascontiguousarray(wave_np)
    if x.dtype != np.int16:
        x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("ctc_pytorch_amd.reverberate_host: expected wave (n), got %s" % (x.shape,))
    n = x.shape[0]
    o = _reverb_opts(rir_prob, noise_prob, normalize)
    out = np.zeros(n, dtype=np.float32)
    _lib.check(_lib.lib().ctcn_reverb_host(_np_ptr(x, n), int(x.dtype == np.int16), n, bank._host_ptr(), ctypes.byref(o), int(seed) & _U64,
                                           int(utt_index) & _U64, _np_ptr(out, n)), "reverberate_host")
    return out


def reverberate(wave, lengths, bank, seed, utt_offset=0, rir_prob=1.0, noise_prob=1.0, normalize=True):
    """Reverberation and additive noise of a padded batch of waveforms (ctcn_reverb; the computation, step by step, in include/ctcn.h): wave
    (B, Nmax) float32 or int16, lengths (B) samples -- a list or a device tensor, clamped to [0, Nmax]; samples at or beyond them are never
    read and come out as zeros.  Utterance b draws from (seed, utt_offset + b) alone: with probability rir_prob one impulse response of
    the bank is convolved into it, with probability noise_prob one noise of the bank, from a drawn offset and repeated as often as needed,
    is added at one of the bank's SNRs against the early part of the reverberated signal; normalize scales the result back to the
    input's power.  Returns out (B, Nmax) float32 on the input's scale, a new tensor.  No autograd; device tensors only (no CPU
    fallback)."""
    _expect("reverberate", bank, ReverbBank)
    if not torch.is_tensor(wave):
        raise ValueError("ctc_pytorch_amd.reverberate: expected wave (B, Nmax), got %s" % type(wave).__name__)
    wave, lens, _ = _wave_batch("reverberate", wave, lengths, also=(lengths,) if torch.is_tensor(lengths) else ())
    (B, Nmax), dev = wave.shape, wave.device
    o = _reverb_opts(rir_prob, noise_prob, normalize)
    L = _lib.lib()
    out = torch.empty((B, Nmax), dtype=torch.float32, device=dev)
    need = L.ctcn_reverb_ws_bytes(bank._host_ptr(), B, Nmax)
    ws = _lib.workspace(dev, nbytes=max(need, 8), tag="reverb")
    _lib.check(L.ctcn_reverb(_ptr(wave) if Nmax else None, int(wave.dtype == torch.int16), _ptr(lens), bank._host_ptr(), _ptr(bank.on(dev)),
                             ctypes.byref(o), int(seed) & _U64, int(utt_offset) & _U64, _ptr(out) if Nmax else None, B, Nmax, _ptr(ws), ws.numel(),
                             _lib.stream_ptr()), "reverberate")
    return out


def cmvn_accumulate(feats, frames, stats):
    """Adds the rows t < frames[b] of feats (B, Tmax, F) float32 to stats (2, F + 1) float64 on the device, Kaldi's CMVN statistics layout
    (sums | count; sums of squares | 0): ctcn_cmvn_accumulate.  Rows at or beyond frames[b] are never read; float64 partial sums combined
    in a fixed order.  Returns stats."""
    _need_gpu(feats, frames, stats)
    if feats.dim() != 3 or feats.dtype != torch.float32:
        raise ValueError("ctc_pytorch_amd.cmvn_accumulate: expected feats (B, Tmax, F) float32, got %s %s" % (tuple(feats.shape), feats.dtype))
    B, Tmax, F = feats.shape
    if frames.numel() != B or stats.dtype != torch.float64 or tuple(stats.shape) != (2, F + 1) or not stats.is_contiguous():
        raise ValueError("ctc_pytorch_amd.cmvn_accumulate: expected frames (%d) and contiguous float64 stats (2, %d)" % (B, F + 1))
    if B == 0 or Tmax == 0:
        return stats
    feats = feats.contiguous()
    frames = frames.to(device=feats.device, dtype=torch.int32).contiguous()
    need = _lib.lib().ctcn_cmvn_accumulate_ws_bytes(B, Tmax, F)
    ws = _lib.workspace(feats.device, nbytes=need, tag="cmvn")
    _lib.check(_lib.lib().ctcn_cmvn_accumulate(_ptr(feats), _ptr(frames), _ptr(stats), B, Tmax, F, _ptr(ws), ws.numel(), _lib.stream_ptr()),
               "cmvn_accumulate")
    return stats


# normalisation per group of utterances and over a sliding window (cmvn.hip): Kaldi's per-speaker CMVN and apply-cmvn-sliding
SLIDING_CMN_OPTIONS = dict(cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False)
_sliding_opts = _StructFrom(_lib.SlidingCmnOpts, SLIDING_CMN_OPTIONS)


def _cmvn_groups(who, groups, B, G, device):
    """Group ids as an int32 device tensor; a host sequence is range-checked here, a device tensor is taken as it is (ids outside [0, G)
    are skipped by the kernels)."""
    if torch.is_tensor(groups) and groups.is_cuda:
        ids = groups.to(device=device, dtype=torch.int32).contiguous()
    else:
        host = [int(v) for v in (groups.tolist() if torch.is_tensor(groups) else groups)]
        bad = [v for v in host if not 0 <= v < G]
        if bad:
            raise ValueError("ctc_pytorch_amd.%s: group id %d outside [0, %d)" % (who, bad[0], G))
        ids = torch.as_tensor(host, dtype=torch.int32).to(device)
    if ids.numel() != B:
        raise ValueError("ctc_pytorch_amd.%s: %d group ids for a batch of %d" % (who, ids.numel(), B))
    return ids


def _group_stats(who, stats, F, shapes):
    if stats.dtype != torch.float64 or stats.dim() != 3 or tuple(stats.shape[1:]) != (2, F + 1) or stats.shape[0] < 1 or not stats.is_contiguous():
        raise ValueError("ctc_pytorch_amd.%s: expected contiguous float64 stats %s, got %s %s" % (who, shapes % {"F1": F + 1}, tuple(stats.shape), stats.dtype))
    return stats.shape[0]


def _out_like(who, feats, out):
    """`out` checked against feats (float32, its shape and device, contiguous), or a new tensor."""
    if out is None:
        return torch.empty(tuple(feats.shape), dtype=torch.float32, device=feats.device)
    if out.dtype != torch.float32 or out.shape != feats.shape or not out.is_contiguous() or out.device != feats.device:
        raise ValueError("ctc_pytorch_amd.%s: out must be a contiguous float32 tensor of feats' shape %s on its device" % (who, tuple(feats.shape)))
    return out


def cmvn_accumulate_groups(feats, frames, groups, stats):
    """Adds the rows t < frames[b] of utterance b of feats (B, Tmax, F) float32 to stats[groups[b]]; stats (G, 2, F + 1) float64 on the device,
    one Kaldi statistics matrix per group (a speaker; or the utterance itself): ctcn_cmvn_accumulate_groups.  groups: B ids as a host
    sequence (range-checked here) or a device tensor (an id outside [0, G) contributes nothing).  Rows at or beyond frames[b] are never
    read; float64 partial sums combined in a fixed order.  Returns stats."""
    frames = _feature_batch("cmvn_accumulate_groups", feats, frames, dtype_error=ValueError)
    _need_gpu(stats)
    B, Tmax, F = feats.shape
    G = _group_stats("cmvn_accumulate_groups", stats, F, "(G, 2, %(F1)d)")
    ids = _cmvn_groups("cmvn_accumulate_groups", groups, B, G, feats.device)
    if B == 0 or Tmax == 0:
        return stats
    feats = feats.contiguous()
    need = _lib.lib().ctcn_cmvn_accumulate_ws_bytes(B, Tmax, F)
    ws = _lib.workspace(feats.device, nbytes=need, tag="cmvn")
    _lib.check(_lib.lib().ctcn_cmvn_accumulate_groups(_ptr(feats), _ptr(frames), _ptr(ids), _ptr(stats), B, Tmax, F, G, _ptr(ws), ws.numel(),
                                                      _lib.stream_ptr()), "cmvn_accumulate_groups")
    return stats


def cmvn_apply(feats, frames, stats, groups=None, norm_vars=True, out=None):
    """(x - mean) * scale with the mean and 1 / stddev of the utterance's group, formed on the device from stats (ctcn_cmvn_apply; the
    formulas of GlobalCMVN.mean_scale): feats (B, Tmax, F) float32, stats (G, 2, F + 1) float64 or one (2, F + 1) matrix.  groups: B ids
    (host sequence, range-checked; or device tensor, an id outside [0, G) copies its utterance through); None: group 0 for all.
    norm_vars False: means only.  Rows at or beyond frames[b] are never read and come out as zeros.  out: a contiguous tensor of
    feats' shape, which may be feats itself (in place); None: a new tensor.  Returns out."""
    frames = _feature_batch("cmvn_apply", feats, frames, dtype_error=ValueError)
    _need_gpu(stats, out)
    B, Tmax, F = feats.shape
    G = _group_stats("cmvn_apply", stats.unsqueeze(0) if stats.dim() == 2 else stats, F, "(G, 2, %(F1)d) or (2, %(F1)d)")
    ids = None if groups is None else _cmvn_groups("cmvn_apply", groups, B, G, feats.device)
    out = _out_like("cmvn_apply", feats, out)
    if B == 0 or Tmax == 0 or F == 0:
        return out
    if out.data_ptr() == feats.data_ptr() and not feats.is_contiguous():
        raise ValueError("ctc_pytorch_amd.cmvn_apply: in-place use needs contiguous feats")
    feats = feats.contiguous()
    _lib.check(_lib.lib().ctcn_cmvn_apply(_ptr(feats), _ptr(frames), _ptr(ids), _ptr(stats), _ptr(out), B, Tmax, F, G, int(bool(norm_vars)),
                                          _lib.stream_ptr()), "cmvn_apply")
    return out


def cmvn_sliding_run(cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False):
    """Frames the sliding-window kernel stages at a time under these options (ctcn_cmvn_sliding_run).  RuntimeError for options the kernel
    refuses.  No device."""
    opts = _sliding_opts(cmn_window, min_cmn_window, normalize_variance, center)
    return _checked(_lib.lib().ctcn_cmvn_sliding_run(ctypes.byref(opts)), "cmvn_sliding_run")


def cmvn_sliding_window(t, n, cmn_window=600, min_cmn_window=100, center=False):
    """(start, end) of the window of frame t in an utterance of n frames, Kaldi's SlidingWindowCmn rule (ctcn_cmvn_sliding_window).  Host
    arithmetic, no device.  RuntimeError for bad arguments."""
    s, e = ctypes.c_int32(), ctypes.c_int32()
    opts = _sliding_opts(cmn_window, min_cmn_window, False, center)
    _lib.check(_lib.lib().ctcn_cmvn_sliding_window(int(t), int(n), ctypes.byref(opts), ctypes.byref(s), ctypes.byref(e)), "cmvn_sliding_window")
    return s.value, e.value


def cmvn_sliding_host(feats_np, cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False, out=None):
    """cmvn_sliding for ONE utterance on the host (ctcn_cmvn_sliding_host: the arithmetic the kernel is compiled from): feats_np (T, F)
    float32 numpy -> a (T, F) float32 array (`out`, which must not overlap the input, or a new one).  No device."""
    x = np.ascontiguousarray(feats_np, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] == 0:
        raise ValueError("ctc_pytorch_amd.cmvn_sliding_host: expected feats (T, F), got %s" % (x.shape,))
    T, F = x.shape
    if out is None:
        out = np.empty_like(x)
    elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != x.shape or not out.flags.c_contiguous:
        raise ValueError("ctc_pytorch_amd.cmvn_sliding_host: out must be a contiguous float32 array of shape %s" % (x.shape,))
    opts = _sliding_opts(cmn_window, min_cmn_window, normalize_variance, center)
    _lib.check(_lib.lib().ctcn_cmvn_sliding_host(_np_ptr(x, T), T, F, ctypes.byref(opts), _np_ptr(out, T)), "cmvn_sliding_host")
    return out


def cmvn_norm_host(stats_np, norm_vars=True):
    """(mean, scale) float32 arrays of ONE statistics matrix (2, F + 1) on the host (ctcn_cmvn_norm_host: the arithmetic cmvn_apply is
    compiled from).  No device.  RuntimeError where no frames are accumulated."""
    s = np.ascontiguousarray(stats_np, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 2 or s.shape[1] < 2:
        raise ValueError("ctc_pytorch_amd.cmvn_norm_host: expected stats (2, F + 1), got %s" % (s.shape,))
    F = s.shape[1] - 1
    mean, scale = np.empty(F, dtype=np.float32), np.empty(F, dtype=np.float32)
    _lib.check(_lib.lib().ctcn_cmvn_norm_host(_np_ptr(s), F, int(bool(norm_vars)), _np_ptr(mean), _np_ptr(scale)), "cmvn_norm_host")
    return mean, scale


def cmvn_sliding(feats, frames, cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False, out=None):
    """Kaldi's apply-cmvn-sliding on a zero-padded batch in one launch (ctcn_cmvn_sliding; the window rule and the running sums, step by
    step, in include/ctcn.h): feats (B, Tmax, F) float32, frames (B) the utterances' frame counts -- a list or a device tensor, clamped to
    [0, Tmax]; rows at or beyond them are never read and come out as zeros.  Options and defaults are Kaldi's.  Returns out (B, Tmax, F)
    float32: a new tensor, or `out`, which must not overlap feats.  No autograd; device tensors only (no CPU fallback)."""
    frames = _feature_batch("cmvn_sliding", feats, frames, dtype_error=ValueError)
    _need_gpu(out)
    B, Tmax, F = feats.shape
    opts = _sliding_opts(cmn_window, min_cmn_window, normalize_variance, center)
    if opts.cmn_window < 1 or not 1 <= opts.min_cmn_window <= opts.cmn_window:
        raise ValueError("ctc_pytorch_amd.cmvn_sliding: cmn_window >= 1 and 1 <= min_cmn_window <= cmn_window needed, got %d and %d"
                         % (opts.cmn_window, opts.min_cmn_window))
    out = _out_like("cmvn_sliding", feats, out)
    if B == 0 or Tmax == 0 or F == 0:
        return out
    feats = feats.contiguous()
    _lib.check(_lib.lib().ctcn_cmvn_sliding(_ptr(feats), _ptr(frames), _ptr(out), B, Tmax, F, ctypes.byref(opts), _lib.stream_ptr()), "cmvn_sliding")
    return out


# pitch features (pitch.hip): Kaldi's compute-kaldi-pitch-feats and process-kaldi-pitch-feats
PITCH_OPTIONS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, preemphasis_coefficient=0.0, min_f0=50.0, max_f0=400.0,
                     soft_min_f0=10.0, penalty_factor=0.1, lowpass_cutoff=1000.0, resample_frequency=4000.0, delta_pitch=0.005,
                     nccf_ballast=7000.0, lowpass_filter_width=1, upsample_filter_width=5, snip_edges=True)
PITCH_PROCESS_OPTIONS = dict(pitch_scale=2.0, pov_scale=2.0, pov_offset=0.0, delta_pitch_scale=10.0, delta_pitch_noise_stddev=0.005,
                             normalization_left_context=75, normalization_right_context=75, delta_window=2, delay=0, add_pov_feature=True,
                             add_normalized_log_pitch=True, add_delta_pitch=True, add_raw_log_pitch=False)
_pitch_opts = _StructFrom(_lib.PitchOpts, PITCH_OPTIONS)
_pitch_process_opts = _StructFrom(_lib.PitchProcessOpts, PITCH_PROCESS_OPTIONS)


class PitchPlan(_Plan):
    """The plan of one pitch configuration (ctcn_pitch_plan; Kaldi's PitchExtractionOptions under their names, PITCH_OPTIONS the defaults):
    the geometric lags, the sparse upsampling table and the Viterbi's penalty table, built on the host when the object is made -- a
    RuntimeError here, before any launch, for what the kernels do not take (snip_edges=false, min_f0 >= max_f0, more than 1024 lags, a
    lowpass_cutoff above the lower Nyquist frequency, a preemphasis) -- with the ResamplePlan of step 1, and uploaded once per device on
    first use.  `host` is the block as uint32 words (layout in include/ctcn.h); lags, pitch (S) float32, tap_first, tap_count (S) int32,
    weights (S, stride) float32, soft_lag, penalty (S) float64 are numpy views of it; first_lag, last_lag, window, shift, run as there."""
    _name = "pitch"
    _upload = np.int64                                                 # (8-byte aligned: the block holds doubles)
    _min_words = 8

    def __init__(self, **options):
        buf = self._build(_pitch_opts.keywords("PitchPlan", options))
        opts, hdr = self.opts, buf[:16].view(np.int32)
        self.num_lags, self.first_lag, self.last_lag, self.window, self.shift, self.stride, self.run = (int(v) for v in hdr[:7])
        S, p = self.num_lags, 16
        self.lags = buf[p:p + S].view(np.float32); p += S
        self.pitch = buf[p:p + S].view(np.float32); p += S
        self.tap_first = buf[p:p + S].view(np.int32); p += S
        self.tap_count = buf[p:p + S].view(np.int32); p += S
        self.weights = buf[p:p + S * self.stride].view(np.float32).reshape(S, self.stride); p += S * self.stride
        p += p & 1
        self.soft_lag = buf[p:p + 2 * S].view(np.float64); p += 2 * S
        self.penalty = buf[p:p + 2 * S].view(np.float64)
        self.sample_frequency, self.resample_frequency = int(opts.sample_frequency), int(opts.resample_frequency)
        self.resample_plan = ResamplePlan(self.sample_frequency, self.resample_frequency, num_zeros=int(opts.lowpass_filter_width),
                                          cutoff=float(opts.lowpass_cutoff))

    def frames_of(self, downsampled):
        """Frames of `downsampled` samples at resample_frequency: 0 below one window, else (M - W) / shift + 1 (the rule of pitch.hip)."""
        return (downsampled - self.window) // self.shift + 1 if downsampled >= self.window else 0

    def num_frames(self, num_samples):
        return self.frames_of(self.resample_plan.num_samples(num_samples))


def pitch_frames(num_samples, plan):
    """Pitch frames of a signal of num_samples samples at plan.sample_frequency (ctcn_pitch_frames: M = ceil(N rf / fs) downsampled samples,
    0 frames for M < W, else (M - W) / shift + 1 -- up to one more than the filterbank's count).  Host arithmetic, no device."""
    _expect("pitch_frames", plan, PitchPlan)
    r = _lib.lib().ctcn_pitch_frames(int(num_samples), ctypes.byref(plan.opts))
    if r < 0:
        raise ValueError("ctc_pytorch_amd.pitch_frames: bad sample count %r" % (num_samples,))
    return r


def pitch(wave, lengths, plan, return_lags=False):
    """Kaldi's compute-kaldi-pitch-feats on a padded batch (ctcn_resample, then ctcn_pitch; the computation, step by step, in
    include/ctcn.h): wave (B, Nmax) float32 or int16 at plan.sample_frequency, lengths (B) samples, a list or a tensor (read on the host),
    plan a PitchPlan.  Returns (raw (B, Tmax, 2) float32: [NCCF for the probability of voicing, pitch in Hz] per frame, rows from frames[b]
    on zero; frames (B) int32) and, with return_lags, the chosen lag index per frame (B, Tmax) int32.  No autograd; device tensors only (no
    CPU fallback)."""
    _expect("pitch", plan, PitchPlan)
    down, lens = resample(wave, lengths, plan.resample_plan)
    (B, Mmax), dev = down.shape, down.device
    Tmax = max(plan.frames_of(m) for m in lens)
    lens_t = torch.as_tensor(lens, dtype=torch.int32).to(dev)
    raw = torch.empty((B, Tmax, 2), dtype=torch.float32, device=dev)
    lags = torch.empty((B, Tmax), dtype=torch.int32, device=dev) if return_lags else None
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    L = _lib.lib()
    need = L.ctcn_pitch_workspace_bytes(ctypes.byref(plan.opts), B, Tmax)
    ws = _lib.workspace(dev, nbytes=need, tag="pitch")
    _lib.check(L.ctcn_pitch(_ptr(down) if Mmax else None, _ptr(lens_t), ctypes.byref(plan.opts), _ptr(plan.on(dev)), _ptr(raw) if Tmax else None,
                            _ptr(lags) if return_lags and Tmax else None, _ptr(frames), B, Mmax, Tmax, _ptr(ws), ws.numel(), _lib.stream_ptr()),
               "pitch")
    return (raw, frames, lags) if return_lags else (raw, frames)


def pitch_host(wave_np, plan, return_lags=False):
    """compute-kaldi-pitch-feats for ONE utterance on the host (ctcn_resample_host, then ctcn_pitch_host: the arithmetic the kernels are
    compiled from): wave_np (N) float32 or int16 numpy at plan.sample_frequency -> raw (T, 2) float32 (and the lag indices (T) int32).
    No device."""
    _expect("pitch_host", plan, PitchPlan)
    x = np.ascontiguousarray(wave_np)
    if x.ndim != 1 or x.dtype not in (np.float32, np.int16):
        raise ValueError("ctc_pytorch_amd.pitch_host: expected a 1-D float32 or int16 waveform")
    L, rp, N = _lib.lib(), plan.resample_plan, x.shape[0]
    M = rp.num_samples(N)
    down = np.zeros(max(M, 1), dtype=np.float32)
    _checked(L.ctcn_resample_host(_np_ptr(x, N), int(x.dtype == np.int16), N, ctypes.byref(rp.opts), rp._host_ptr(), _np_ptr(down), down.shape[0]),
             "resample_host")
    T = plan.frames_of(M)
    raw, lags = np.zeros((T, 2), dtype=np.float32), np.zeros(T, dtype=np.int32)
    _checked(L.ctcn_pitch_host(_np_ptr(down), M, ctypes.byref(plan.opts), plan._host_ptr(), _np_ptr(raw, T), _np_ptr(lags, T), T), "pitch_host")
    return (raw, lags) if return_lags else raw


def _process_opts(who, options):
    opts = _pitch_process_opts.keywords(who, options)
    cols = sum(int(bool(getattr(opts, k))) for k in ("add_pov_feature", "add_normalized_log_pitch", "add_delta_pitch", "add_raw_log_pitch"))
    if cols == 0:
        raise ValueError("ctc_pytorch_amd.%s: every column is switched off" % who)
    if not float(opts.delta_pitch_noise_stddev) >= 0.0:
        raise ValueError("ctc_pytorch_amd.%s: delta_pitch_noise_stddev must not be negative" % who)
    return opts, cols


def pitch_process(raw, frames, seed=0, utt_offset=0, **options):
    """Kaldi's process-kaldi-pitch-feats on a zero-padded batch in one launch (ctcn_pitch_process; Kaldi's ProcessPitchOptions under their
    names, PITCH_PROCESS_OPTIONS the defaults): raw (B, Tmax, 2) float32 as pitch returns it, frames (B) a list or a device tensor.
    Returns (B, Tmax, C) float32, C = 3 under the defaults: POV feature, normalised log pitch, delta log pitch (, raw log pitch); rows at or
    beyond frames[b] zero.  The delta's noise is a function of (seed, b + utt_offset, frame) alone.  RuntimeError for a delay."""
    opts, cols = _process_opts("pitch_process", options)
    if raw.dim() != 3 or raw.shape[2] != 2 or raw.dtype != torch.float32:
        raise ValueError("ctc_pytorch_amd.pitch_process: expected raw (B, Tmax, 2) float32, got %s %s" % (tuple(raw.shape), raw.dtype))
    frames = _feature_batch("pitch_process", raw, frames, dtype_error=ValueError)
    B, Tmax, _ = raw.shape
    out = torch.empty((B, Tmax, cols), dtype=torch.float32, device=raw.device)
    if Tmax == 0:
        _lib.check(_lib.lib().ctcn_pitch_process_host(None, 0, ctypes.byref(opts), 0, 0, None) - cols, "pitch_process")      # (the refusals)
        return out
    raw = raw.contiguous()
    _lib.check(_lib.lib().ctcn_pitch_process(_ptr(raw), _ptr(frames), ctypes.byref(opts), _ptr(out), B, Tmax, int(seed) & _U64, int(utt_offset),
                                             _lib.stream_ptr()), "pitch_process")
    return out


def pitch_process_host(raw_np, seed=0, utt_index=0, **options):
    """pitch_process for ONE utterance on the host (ctcn_pitch_process_host): raw_np (T, 2) float32 numpy -> (T, C) float32.  No device."""
    opts, cols = _process_opts("pitch_process_host", options)
    x = np.ascontiguousarray(raw_np, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("ctc_pytorch_amd.pitch_process_host: expected raw (T, 2), got %s" % (x.shape,))
    T = x.shape[0]
    out = np.zeros((T, cols), dtype=np.float32)
    _checked(_lib.lib().ctcn_pitch_process_host(_np_ptr(x, T), T, ctypes.byref(opts), int(seed) & _U64, int(utt_index), _np_ptr(out, T)),
             "pitch_process_host")
    return out
