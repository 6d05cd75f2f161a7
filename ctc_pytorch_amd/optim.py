"""Flat parameter / gradient storage and fused Adam for the HIP path.

replaces: torch.optim.Adam(model.parameters(), lr, weight_decay) as used at the reference's
timit/steps/train_ctc.py:145,62-65 (L2-coupled weight decay, betas (0.9,0.999), eps 1e-8).

All parameters of the model are re-homed into ONE contiguous float32 buffer and all gradients into a second
one (288 GB of HBM: no reason to scatter 25 tensors), each parameter starting on 16 bytes (flat_layout).  The backward kernels of ops.py accumulate weight
gradients straight into views of the flat gradient buffer (`param._ctcn_grad`), so a training step needs
  1 memset (zero_grad) + 1 RCCL all-reduce over the flat gradient (data parallel) + 1 fused Adam launch.
BatchNorm running statistics stay ordinary buffers.
"""
import torch

from . import _lib, ops


def placement_order(names):
    """Indices of `names` (model.named_parameters() order) in flat-buffer placement order: unchanged, except that inside each
    module the recurrent weights come as weight_ih_l0, weight_ih_l0_reverse, weight_hh_l0, weight_hh_l0_reverse."""
    rank = {"weight_ih_l0": 0, "weight_ih_l0_reverse": 1, "weight_hh_l0": 2, "weight_hh_l0_reverse": 3}
    first = {}
    for i, n in enumerate(names):
        first.setdefault(n.rsplit(".", 1)[0], i)
    return sorted(range(len(names)), key=lambda i: (first[names[i].rsplit(".", 1)[0]], rank.get(names[i].rsplit(".", 1)[-1], 4), i))


ALIGN = 4      # floats: every parameter starts on 16 bytes inside the (allocator-aligned) flat buffers


def flat_layout(sizes):
    """(offsets, total) of tensors of `sizes` elements placed in that order in a flat buffer: back to back, each start rounded up to a
    multiple of ALIGN elements -- the operand alignment the recurrent kernels require of W_hh (DESIGN, "Operand alignment contract") and
    the vector paths of all the others take.  Sizes that are all multiples of ALIGN (every shipped configuration) give the plain prefix
    sums; the padding elements belong to no parameter and hold zero in every buffer.  Device-free."""
    offsets, off = [], 0
    for n in sizes:
        off = -(-off // ALIGN) * ALIGN
        offsets.append(off)
        off += int(n)
    return offsets, off


class FlatAdam:
    """Adam over the flattened parameters of `model`; same public surface as torch.optim.Optimizer where the
    reference touches it: zero_grad(), step(), state_dict(), load_state_dict(), param_groups[i]['lr']."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, norm_type=2.0, skip_nonfinite=False):
        """max_grad_norm: clip the global gradient norm (norm_type 2 or inf) to it inside step(), torch's clip_grad_norm_ expression; the
        gradient buffer itself is NOT rewritten (Adam applies the coefficient while it reads it -- clip_grad_norm_() below is the form that
        leaves clipped gradients behind).  skip_nonfinite: a step whose gradient holds a NaN or Inf is dropped -- parameters, moments and
        the bias-correction count stay as they were (what torch.amp.GradScaler.step does) -- and counted in `skipped_steps`.  Both off
        (the default): step() is the plain fused Adam, the same launch as without these arguments.  Neither synchronises with the host."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("FlatAdam: max_grad_norm must be > 0 (or None), got %r" % (max_grad_norm,))
        ops.norm_type_code(norm_type)                # NotImplementedError for anything but 2 and inf
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.norm_type = float(norm_type)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ctl = self._norm_ws = None             # device control block (ctcn_clip_ctl) / norm workspace, made on the first guarded step
        self._clip_ctl = self._last_norm_ctl = None  # scratch control block of clip_grad_norm_() / the block last_grad_norm reads
        self._ctl_stale, self._host_exact = False, True
        self.model = model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("no parameters")
        # Placement order in the flat buffers: model order, except that the input-projection weights of the two directions of a
        # recurrent layer sit next to each other (weight_ih_l0, weight_ih_l0_reverse, then the two weight_hh): ctcn_rnn_fwd /
        # ctcn_rnn_bwd then see [W_ih_fwd ; W_ih_rev] as ONE (2*G*H, I) matrix and run the input projection / dx as a single
        # product without stacking copies.  `self.params` keeps the model's own order.
        placed = placement_order([n for n, _ in named])
        self.layout = [named[i][0] for i in placed]
        params = [named[i][1] for i in placed]
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdam: move the model to the ROCm device first (no CPU path)")
        self.params = [p for _, p in named]
        sizes = [p.numel() for p in params]
        self.offsets, total = flat_layout(sizes)
        # zeros, not empty: a padding element is 0 in all four buffers and stays 0 (Adam of p = g = m = v = 0 is 0, with weight decay and
        # any clip coefficient; no backward kernel writes outside a parameter's view; the gradient norm does not see a zero)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, n, off in zip(params, sizes, self.offsets):
                self.flat[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.flat[off:off + n].view(p.shape)
                g = self.grad[off:off + n].view(p.shape)
                p._ctcn_grad = g          # ops.py backward kernels accumulate here and return None to autograd
                p.grad = g
        self.step_count = 0
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, params=self.params)]

    def zero_grad(self, set_to_none=False):
        ops.join_side_stream()            # no-op unless weight gradients are still in flight on the side stream
        self.grad.zero_()

    # ---- the number of APPLIED steps (Adam's bias-correction count).  One rule: the host integer is exact unless a GUARDED step ran since it
    # was last read -- only the device knows whether that step was dropped -- and then the next read fetches the device counter (a sync),
    # whatever max_grad_norm / skip_nonfinite are set to by then (both are plain attributes and may be switched on a live optimiser).
    # A value written from the host (load_state_dict, a plain step) goes to the device counter before the next clipped / guarded step. ----
    @property
    def step_count(self):
        if not self._host_exact:
            self._step_host = int(self._ctl[ops.CTL_STEP].item())
            self._host_exact = True
        return self._step_host

    @step_count.setter
    def step_count(self, value):
        self._step_host = int(value)
        self._host_exact = True
        self._ctl_stale = self._ctl is not None

    @property
    def skipped_steps(self):
        """Steps the guard has dropped so far (reads the device counter: synchronises)."""
        return 0 if self._ctl is None else int(self._ctl[ops.CTL_SKIPPED].item())

    @property
    def last_grad_norm(self):
        """Global gradient norm measured by the last clipped / guarded step() or the last clip_grad_norm_(), before clipping: a 0-d DEVICE
        tensor (a view of a control block: read it, or clone it, before the next such call), None before the first one."""
        return None if self._last_norm_ctl is None else self._last_norm_ctl.view(torch.float32)[ops.CTL_NORM]

    def _control(self):
        if self._ctl is None:
            self._ctl = ops.new_clip_ctl(self.grad.device, step=self._step_host)
            need = _lib.lib().ctcn_grad_norm_ws_bytes(self.grad.numel(), 0)
            self._norm_ws = torch.empty(max(int(need), 8), dtype=torch.uint8, device=self.grad.device)
        elif self._ctl_stale:                # the host count moved (load_state_dict, plain steps) since the device counter was written
            self._ctl[ops.CTL_STEP] = self.step_count
        self._ctl_stale = False
        return self._ctl

    def clip_grad_norm_(self, max_norm, norm_type=None, error_if_nonfinite=False):
        """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) on the flat gradient: joins the side stream, returns the pre-clip norm
        (0-d device tensor) and leaves the clipped gradients in the buffer, for callers who want torch's two-call shape.  It has a scratch
        control block of its own (made once): the step bookkeeping of step() is not touched."""
        ops.join_side_stream()
        if self._clip_ctl is None:
            self._clip_ctl = ops.new_clip_ctl(self.grad.device)
        self._last_norm_ctl = self._clip_ctl
        return ops.clip_grad_norm_(self.grad, max_norm, self.norm_type if norm_type is None else norm_type, error_if_nonfinite, ctl=self._clip_ctl)

    def step(self):
        ops.join_side_stream()
        g = self.param_groups[0]
        if self.max_grad_norm is None and not self.skip_nonfinite:
            self.step_count += 1
            ops.adam_step(self.flat, self.grad, self.m, self.v, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                          self._step_host)
            return
        # norm -> clip decision and step bookkeeping -> Adam reading them, all on the device: no host sync, no extra pass over the gradient.
        # Data parallel: the buffer is the all-reduced one, bit-identical on every rank, and the norm is a function of its bits alone, so
        # every rank takes the same decision with the same coefficient and no further collective.
        ctl = self._control()
        ops.grad_norm(self.grad, self.norm_type, ctl=ctl, ws=self._norm_ws)
        ops.clip_control(ctl, float("inf") if self.max_grad_norm is None else self.max_grad_norm, g["lr"], g["betas"][0], g["betas"][1],
                         self.skip_nonfinite)
        ops.adam_step_ex(self.flat, self.grad, self.m, self.v, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], ctl)
        self._last_norm_ctl = ctl
        if self.skip_nonfinite:
            self._host_exact = False         # the device decided whether this step counts: step_count reads its counter on demand
        else:
            self._step_host += 1             # (one behind the truth by the same amount as before if _host_exact is already False)

    # ---- checkpoint surface: the torch.optim.Adam layout, so that 'optim_dict' of a package written by either side loads in
    # the other (train_ctc.py:198,223,246 snapshot / roll back / save optimizer.state_dict()) ---------------------------------
    def _slices(self):
        """(index in model.parameters() order, offset, numel, shape) of every parameter inside the flat buffers."""
        order = {id(p): i for i, p in enumerate(self.params)}
        by_name = dict((n, p) for n, p in self.model.named_parameters() if p.requires_grad)
        ps = [by_name[name] for name in self.layout]
        return [(order[id(p)], off, p.numel(), tuple(p.shape)) for p, off in zip(ps, self.offsets)]

    def state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} exactly as torch.optim.Adam writes it
        (parameter i = i-th of model.parameters()); the moments are per-parameter copies of the flat buffers."""
        g = self.param_groups[0]
        template = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"],
                                    weight_decay=g["weight_decay"]).state_dict()["param_groups"][0]      # key set of this torch version
        group = dict(template, params=list(range(len(self.params))))
        state = {}
        steps = self.step_count                  # applied steps: with the guard on, read from the device counter (a dropped step does not count)
        if steps > 0:
            for i, off, n, shape in self._slices():
                state[i] = {"step": torch.tensor(float(steps)), "exp_avg": self.m[off:off + n].view(shape).clone(),
                            "exp_avg_sq": self.v[off:off + n].view(shape).clone()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        if "state" not in sd and "m" in sd:            # round-1 packages: flat moment buffers
            if "layout" in sd and list(sd["layout"]) != list(self.layout):
                raise ValueError("FlatAdam.load_state_dict: the moment buffers were saved with a different parameter placement")
            self.step_count = int(sd["step"])
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
        else:
            groups = sd["param_groups"]
            if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
                raise ValueError("FlatAdam.load_state_dict: expected one parameter group over %d parameters" % len(self.params))
            state, steps = sd["state"], set()
            self.m.zero_()
            self.v.zero_()
            for i, off, n, shape in self._slices():
                st = state.get(i, state.get(str(i)))
                if st is None:
                    continue
                if tuple(st["exp_avg"].shape) != shape:
                    raise ValueError("FlatAdam.load_state_dict: parameter %d has shape %s, the checkpoint %s" % (i, shape, tuple(st["exp_avg"].shape)))
                self.m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                self.v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(float(st["step"])))
            if len(steps) > 1:
                raise ValueError("FlatAdam.load_state_dict: per-parameter step counts differ (%s); one fused step serves all" % sorted(steps))
            self.step_count = steps.pop() if steps else 0
        for k, v in sd["param_groups"][0].items():
            if k in ("lr", "betas", "eps", "weight_decay"):
                self.param_groups[0][k] = v
