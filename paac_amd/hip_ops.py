"""Thin, shape-checked Python wrappers over the C-ABI (include/paac_hip.h).

torch is plumbing only (device memory + streams): every wrapper validates dtype / device / contiguity /
extent on the host BEFORE the launch (a kernel that faults can take the whole node down), then hands raw
device pointers to libpaac_hip.so on torch's current HIP stream.
"""
import ctypes
import functools
import gc

import numpy as np
import torch

from . import _lib

OBS_SHAPE = (84, 84, 4)
RAW_H, RAW_W = 210, 160
FINISHED_RING_BYTES = 8 + 4096 * 4 + 4096 * 4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype, numel=None, name="tensor", optional=False):
    if t is None:
        if optional:
            return ctypes.c_void_p(0)
        raise ValueError("%s is required" % name)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s must be a CUDA/HIP torch tensor" % name)
    if t.dtype != dtype:
        raise ValueError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if numel is not None and t.numel() < numel:
        raise ValueError("%s: %d elements, need >= %d" % (name, t.numel(), numel))
    return ctypes.c_void_p(t.data_ptr())


def _lent(t):
    """(pointer, bytes) of an optional uint8 scratch tensor."""
    return (ctypes.c_void_p(t.data_ptr()), int(t.numel())) if t is not None else (ctypes.c_void_p(0), 0)


def _step_ptrs(N, stack_out=None, rewards_out=None, masks_out=None, ep_reward=None, ep_len=None, finished=None, stack_out2=None,
               stack_in=None, states=None):
    """What one environment step of N environments writes, as every step entry takes it (csrc/synth_dev.h: SynthStep), in the C
    order: stack_out, stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished -- behind the checks the entries share.
    stack_in: the stacks a separate step reads (shape-checked here, passed by the entry); states: the observations an entry
    that also runs the policy reads, which its step cannot shift in place.  No stack_out: no environment step, seven nulls."""
    if stack_out is None:
        return [ctypes.c_void_p(0)] * 7
    for nm, t in (("stack_in", stack_in), ("stack_out", stack_out), ("stack_out2", stack_out2)):
        if t is not None and tuple(t.shape) != (N,) + OBS_SHAPE:
            raise ValueError("%s must be [%d,84,84,4], got %s" % (nm, N, tuple(t.shape)))
    if states is not None and states.data_ptr() in [t.data_ptr() for t in (stack_out, stack_out2) if t is not None]:
        raise ValueError("the step cannot shift the stacks in place")
    if finished is not None and finished.numel() * finished.element_size() < FINISHED_RING_BYTES:
        raise ValueError("finished ring too small")
    return [_ptr(stack_out, torch.uint8, N * 28224, "stack_out"), _ptr(stack_out2, torch.uint8, N * 28224, "stack_out2", True),
            _ptr(rewards_out, torch.float32, N, "rewards_out"), _ptr(masks_out, torch.float32, N, "masks_out"),
            _ptr(ep_reward, torch.float32, N, "ep_reward"), _ptr(ep_len, torch.int32, N, "ep_len"),
            ctypes.c_void_p(finished.data_ptr()) if finished is not None else ctypes.c_void_p(0)]


# The buffer checks of the device games' wrappers (game / duel / ghost steps and resets, eval_step, match_step).
def _shaped_ptrs(shape, dtype, named, nullable):
    """Every named tensor against `shape` -> their pointers in the order given; the names in `nullable` may be None."""
    for nm, t in named.items():
        if t is not None and tuple(t.shape) != shape:
            raise ValueError("%s must be [%s], got %s" % (nm, ",".join(str(d) for d in shape), tuple(t.shape)))
    return [_ptr(t, dtype, int(np.prod(shape)), nm, nm in nullable) for nm, t in named.items()]


def _state_ptrs(N, words, nullable=(), **named):
    """int32 state records [N, words]."""
    return _shaped_ptrs((N, words), torch.int32, named, nullable)


def _stack_ptrs(N, nullable=(), **named):
    """uint8 observation stacks [N, 84, 84, 4]."""
    return _shaped_ptrs((N,) + OBS_SHAPE, torch.uint8, named, nullable)


def _env_offset(fn, env_offset, N):
    """The first global environment of N: they all have 32-bit keys."""
    if not 0 <= int(env_offset) <= 0xFFFFFFFF - N:
        raise ValueError("%s: env_offset %r" % (fn, env_offset))
    return int(env_offset)


def _env_records(N, records, truncs_out):
    """paac_env_records: _step_ptrs' five record pointers and the truncation plane float32[N] (None: not written)."""
    return _lib.EnvRecords(*records, _ptr(truncs_out, torch.float32, N, "truncs_out", True))


def _game_step_ptrs(words, actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2, rewards_out, masks_out,
                    ep_reward, ep_len, finished):
    """What the game steps share -> N, [actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2] in the C
    order, and the five record pointers."""
    N = actions.shape[0]
    out, out2, *records = _step_ptrs(N, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, stack_in=stack_in)
    states = _state_ptrs(N, words, ("state_out2",), state_in=state_in, state_out=state_out, state_out2=state_out2)
    return N, [_ptr(actions, torch.int32, N, "actions"), *states, _ptr(stack_in, torch.uint8, N * 28224, "stack_in"), out, out2], records


# (filters, kernel size, stride) of the stock trunks' conv layers and their fc width (networks.py)
STOCK_GEOMETRY = {_lib.ARCH_NATURE: ([(32, 8, 4), (64, 4, 2), (64, 3, 1)], 512),
                  _lib.ARCH_NIPS: ([(16, 8, 4), (32, 4, 2)], 256)}


def arch_geometry(arch):
    """-> (convs [(filters, size, stride), ...], fc width) of `arch` in the loaded library."""
    if int(arch) == _lib.ARCH_USER:
        g = _lib.user_arch()
        if g is None:
            raise _lib.PaacHipError("the loaded library has no user architecture")
        return g
    return STOCK_GEOMETRY[int(arch)]


def activation_size(convs, fc, what, batch):
    """Floats paac_debug_activation copies for `what` (include/paac_hip.h) over `batch` rows of the geometry (convs, fc):
    VALID convolutions over 84 x 84; None for a `what` the geometry does not have."""
    what = int(what)
    if what == 25:
        return int(batch)
    if 21 <= what <= 24:
        what -= 20
    elif 11 <= what <= 14:
        what -= 10
    if what == 4:
        return int(batch) * int(fc)
    if not 1 <= what <= len(convs):
        return None
    size = 84
    for _, k, s in convs[:what]:
        size = (size - k) // s + 1
    return int(batch) * size * size * int(convs[what - 1][0])


class Context(object):
    """Owns one paac_ctx (activation workspace for one network on one GPU)."""

    def __init__(self, arch, num_actions, max_batch, device_index=0):
        self.lib = _lib.load()
        self.arch = int(arch)
        self.num_actions = int(num_actions)
        self.max_batch = int(max_batch)
        self.layout = _lib.param_layout(arch, num_actions)
        cfg = _lib.Cfg(device=int(device_index), arch=self.arch, num_actions=self.num_actions, max_batch=self.max_batch)
        h = ctypes.c_void_p()
        _lib.check(self.lib.paac_create(ctypes.byref(cfg), ctypes.byref(h)), "paac_create")
        self.handle = h
        self.device = torch.device("cuda", device_index)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.paac_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- network ---------------------------------------------------------------------------------
    def _check_states(self, states):
        B = states.shape[0]
        if tuple(states.shape[1:]) != OBS_SHAPE:
            raise ValueError("states must be [B,84,84,4] uint8, got %s" % (tuple(states.shape),))
        if not (0 < B <= self.max_batch):
            raise ValueError("batch %d outside (0, %d]" % (B, self.max_batch))
        return B

    def forward(self, params, states, logits=None, probs=None, values=None):
        B = self._check_states(states)
        A = self.num_actions
        _lib.check(self.lib.paac_forward(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                         _ptr(states, torch.uint8, B * 28224, "states"), B,
                                         _ptr(logits, torch.float32, B * A, "logits", True),
                                         _ptr(probs, torch.float32, B * A, "probs", True),
                                         _ptr(values, torch.float32, B, "values", True), _stream()), "paac_forward")

    def forward_sample(self, params, states, seed, step_base_dev, step_offset, env_offset, actions, probs=None,
                       values=None):
        B = states.shape[0]
        if tuple(states.shape[1:]) != OBS_SHAPE:
            raise ValueError("states must be [B,84,84,4] uint8, got %s" % (tuple(states.shape),))
        if not (0 < B <= self.max_batch):
            raise ValueError("batch %d outside (0, %d]" % (B, self.max_batch))
        A = self.num_actions
        _lib.check(self.lib.paac_forward_sample(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                                _ptr(states, torch.uint8, B * 28224, "states"), B,
                                                _ptr(probs, torch.float32, B * A, "probs", True),
                                                _ptr(values, torch.float32, B, "values", True), int(seed),
                                                _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset),
                                                int(env_offset), _ptr(actions, torch.int32, B, "actions"), _stream()),
                   "paac_forward_sample")

    def forward_sample_synth_step(self, params, states, seed, step_base_dev, step_offset, env_offset, actions, env_seed,
                                  terminal_threshold, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished=None,
                                  probs=None, values=None):
        """forward + counter-based sampler + synthetic env step (path A) in the forward's five launches."""
        B = states.shape[0]
        A = self.num_actions
        if tuple(states.shape[1:]) != OBS_SHAPE or tuple(stack_out.shape) != tuple(states.shape):
            raise ValueError("states / stack_out must be [B,84,84,4] uint8, got %s / %s" %
                             (tuple(states.shape), tuple(stack_out.shape)))
        if not (0 < B <= self.max_batch):
            raise ValueError("batch %d outside (0, %d]" % (B, self.max_batch))
        out, _, *records = _step_ptrs(B, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, states=states)
        _lib.check(self.lib.paac_forward_sample_synth_step(
            self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
            _ptr(states, torch.uint8, B * 28224, "states"), B, _ptr(probs, torch.float32, B * A, "probs", True),
            _ptr(values, torch.float32, B, "values", True), int(seed), _ptr(step_base_dev, torch.int64, 1, "step_base", True),
            int(step_offset), int(env_offset), _ptr(actions, torch.int32, B, "actions"), int(env_seed),
            int(terminal_threshold), out, *records, _stream()), "paac_forward_sample_synth_step")

    def train_forward(self, params, states, values=None):
        B = states.shape[0]
        if tuple(states.shape[1:]) != OBS_SHAPE:
            raise ValueError("states must be [B,84,84,4] uint8, got %s" % (tuple(states.shape),))
        if not (0 < B <= self.max_batch):
            raise ValueError("batch %d outside (0, %d]" % (B, self.max_batch))
        _lib.check(self.lib.paac_train_forward(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                               _ptr(states, torch.uint8, B * 28224, "states"), B,
                                               _ptr(values, torch.float32, B, "values", True), _stream()),
                   "paac_train_forward")

    def train_forward_trunk(self, params, states):
        """Training forward without the heads: the next loss_backward[_returns](forward_done=True) finishes them, inside
        its first launch where it can (include/paac_hip.h: paac_train_forward_trunk)."""
        B = self._check_states(states)
        _lib.check(self.lib.paac_train_forward_trunk(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                                     _ptr(states, torch.uint8, B * 28224, "states"), B, _stream()),
                   "paac_train_forward_trunk")

    def _loss_backward(self, entry, params, states, actions, middle, entropy_beta, grad, loss_out, forward_done, phase,
                       stats=None):
        """One paac_loss_backward* call: every entry takes (handle, params, states, actions), then its own `middle` arguments
        -- a (name, tensor[, optional]) tuple per float32[B] array, anything else as it is --, then (batch, beta, grad,
        loss_out), its statistics output (tensor, floats) if it has one, and (forward_done, phase, stream).  The arrays are
        validated in argument order."""
        B = self._check_states(states)
        args = [self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                _ptr(states, torch.uint8, B * 28224, "states"), _ptr(actions, torch.int32, B, "actions")]
        args += [_ptr(m[1], torch.float32, B, m[0], *m[2:]) if isinstance(m, tuple) else m for m in middle]
        args += [B, float(entropy_beta), _ptr(grad, torch.float32, self.layout["total"], "grad"),
                 _ptr(loss_out, torch.float32, 4, "loss_out", True)]
        if stats is not None:
            args.append(_ptr(stats[0], torch.float32, stats[1], "ppo_stats_out", True))
        _lib.check(getattr(self.lib, entry)(*args, 1 if forward_done else 0, int(phase), _stream()), entry)

    def loss_backward(self, params, states, actions, y, adv, entropy_beta, grad, loss_out=None, forward_done=False,
                      phase=0, p_old_out=None):
        """p_old_out: float32[B], also receives p_old (include/paac_hip.h: paac_loss_backward_record); gradient and loss are
        unchanged."""
        record = p_old_out is not None
        self._loss_backward("paac_loss_backward_record" if record else "paac_loss_backward", params, states, actions,
                            (("y", y), ("adv", adv)) + ((("p_old_out", p_old_out),) if record else ()),
                            entropy_beta, grad, loss_out, forward_done, phase)

    def loss_backward_returns(self, params, states, actions, v_boot, rewards, masks, values, gamma, y_out, adv_out,
                              entropy_beta, grad, loss_out=None, forward_done=False, phase=0, global_step_dev=None,
                              increment=0, initial_lr=0.0, lr_annealing_steps=1, lr_out_dev=None, tick_dev=None, tick_inc=0,
                              gae_lambda=None, p_old_out=None, truncs=None):
        """n-step returns (+ the cycle's schedule bookkeeping) inside the backward's first launch
        (include/paac_hip.h: paac_loss_backward_returns) == nstep_returns_tick followed by loss_backward.
        v_boot=None: the bootstrap values are rows [B, B + N) of the training forward that has already run.
        gae_lambda: None or 1.0 = the n-step return; anything else = GAE(lambda) instead (uses_gae).
        p_old_out: float32[B], also receives p_old (epoch 1 of a --ppo_epochs cycle); gradient and loss are unchanged.
        truncs: float32[T,N] truncation plane of --bootstrap_truncated (include/paac_hip.h: paac_returns); None = off."""
        T, N = rewards.shape
        if T * N != states.shape[0]:
            raise ValueError("rollout records are [%d,%d] but the batch has %d rows" % (T, N, states.shape[0]))
        ret = _returns_struct(v_boot, rewards, masks, values, gamma, y_out, adv_out, global_step_dev, increment, initial_lr,
                              lr_annealing_steps, lr_out_dev, tick_dev, tick_inc, gae_lambda, truncs)
        record = p_old_out is not None          # include/paac_hip.h: paac_loss_backward_returns_record
        self._loss_backward("paac_loss_backward_returns_record" if record else "paac_loss_backward_returns", params, states,
                            actions, (ctypes.byref(ret),) + ((("p_old_out", p_old_out),) if record else ()),
                            entropy_beta, grad, loss_out, forward_done, phase)

    def loss_backward_record(self, params, states, actions, y, adv, p_old_out, entropy_beta, grad, loss_out=None,
                             forward_done=False, phase=0):
        """loss_backward that also writes p_old_out[i] = pi(a_i | s_i) as its own heads computed it (include/paac_hip.h:
        paac_loss_backward_record): epoch 1 of a --ppo_epochs cycle for a caller that computes y / adv itself."""
        if p_old_out is None:
            raise ValueError("loss_backward_record needs p_old_out")
        self.loss_backward(params, states, actions, y, adv, entropy_beta, grad, loss_out, forward_done, phase, p_old_out)

    def loss_backward_ppo(self, params, states, actions, y, adv, p_old, clip_eps, entropy_beta, grad, loss_out=None,
                          ppo_stats_out=None, forward_done=False, phase=0):
        """Epochs 2..K of a --ppo_epochs cycle: the clipped surrogate on the frozen y / adv / p_old (include/paac_hip.h:
        paac_loss_backward_ppo).  ppo_stats_out: float32[2] = {clip_fraction, approx_kl}."""
        self._loss_backward("paac_loss_backward_ppo", params, states, actions,
                            (("y", y), ("adv", adv), ("p_old", p_old), float(clip_eps)),
                            entropy_beta, grad, loss_out, forward_done, phase, stats=(ppo_stats_out, 2))

    def loss_backward_ppo_vclip(self, params, states, actions, y, adv, p_old, v_old, clip_eps, vclip_eps, entropy_beta, grad,
                                loss_out=None, ppo_stats_out=None, forward_done=False, phase=0):
        """loss_backward_ppo with the value-clipped critic term of --ppo_vclip on the frozen v_old (include/paac_hip.h:
        paac_loss_backward_ppo_vclip).  ppo_stats_out: float32[3] = {clip_fraction, approx_kl, value_clip_fraction}."""
        self._loss_backward("paac_loss_backward_ppo_vclip", params, states, actions,
                            (("y", y), ("adv", adv), ("p_old", p_old, True), ("v_old", v_old, True), float(clip_eps),
                             float(vclip_eps)),
                            entropy_beta, grad, loss_out, forward_done, phase, stats=(ppo_stats_out, 3))

    def train_values_into(self, out, batch):
        """out[:batch] = the values the training-side heads computed last (paac_debug_activation(25) into the caller's
        array: one device-to-device copy on the stream, capturable): v_old of a --ppo_vclip cycle, right behind epoch 1."""
        _lib.check(self.lib.paac_debug_activation(self.handle, 25, int(batch), _ptr(out, torch.float32, int(batch), "out"),
                                                  int(batch), _stream()), "paac_debug_activation")

    def record_policy(self, params, actions, batch, p_old_out=None, v_out=None, value_rows=None):
        """--ppo_minibatches' record pass (include/paac_hip.h: paac_record_policy): finishes the heads a trunk-only training
        forward (or kept acting rows) left pending, then p_old_out[:batch] = pi(a_i | s_i) and v_out[:value_rows] = the values
        of the training set's first value_rows rows (default batch; more reaches the appended bootstrap rows).  No gradient."""
        batch = int(batch)
        value_rows = batch if value_rows is None else int(value_rows)
        if not 0 < max(batch, value_rows) <= self.max_batch or batch < 0 or value_rows < 0:
            raise ValueError("record_policy: batch %d / value_rows %d outside (0, %d]" % (batch, value_rows, self.max_batch))
        _lib.check(self.lib.paac_record_policy(
            self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
            _ptr(actions, torch.int32, batch, "actions", p_old_out is None), batch,
            _ptr(p_old_out, torch.float32, batch, "p_old_out", True), _ptr(v_out, torch.float32, value_rows, "v_out", True),
            value_rows, _stream()), "paac_record_policy")

    def returns_norm_tick(self, params, v_boot, rewards, masks, values, gamma, y_out, adv_out, adv_n_out, stats_out=None,
                          global_step_dev=None, increment=0, initial_lr=0.0, lr_annealing_steps=1, lr_out_dev=None,
                          tick_dev=None, tick_inc=0, gae_lambda=None, truncs=None):
        """Returns of either estimator + the cycle's schedule bookkeeping + --adv_norm's normalisation in one launch
        (include/paac_hip.h: paac_returns_norm_tick).  v_boot=None: the bootstrap values are rows [T*N, T*N + N) of the
        training forward that has already run on this ctx (the heads of those rows are finished here when they are pending).
        stats_out: float64[2] = {mean, std}.  truncs: the truncation plane of --bootstrap_truncated, None = off."""
        T, N = rewards.shape
        ret = _returns_struct(v_boot, rewards, masks, values, gamma, y_out, adv_out, global_step_dev, increment, initial_lr,
                              lr_annealing_steps, lr_out_dev, tick_dev, tick_inc, gae_lambda, truncs)
        _lib.check(self.lib.paac_returns_norm_tick(
            self.handle, _ptr(params, torch.float32, self.layout["total"], "params"), ctypes.byref(ret),
            _ptr(adv_n_out, torch.float32, T * N, "adv_n_out"), _ptr(stats_out, torch.float64, 2, "stats_out", True), _stream()),
            "paac_returns_norm_tick")

    def _clip_step(self, entry, params, grad, slots, powers, lr_dev, hyper, clip_norm, clip_mode, grad_scale, gnorm_out,
                   gate=None):
        """One optimizer entry: (params, grad, the rule's slot pair[, Adam's powers], n, lr, the rule's three hyper-parameters,
        clip_norm, clip_mode, grad_scale, gnorm_out[, gate]).  gate: the _kl_gate of a gated entry."""
        n = self.layout["total"]
        tail = () if gate is None else (ctypes.byref(gate),)
        _lib.check(getattr(self.lib, entry)(
            self.handle, _ptr(params, torch.float32, n, "params"), _ptr(grad, torch.float32, n, "grad"),
            *[_ptr(t, torch.float32, n, name) for name, t in slots], *powers, n, _ptr(lr_dev, torch.float32, 1, "lr_dev"),
            *[float(h) for h in hyper], float(clip_norm), int(clip_mode), float(grad_scale),
            _ptr(gnorm_out, torch.float32, 1, "gnorm_out", True), *tail, _stream()), entry)

    def clip_rmsprop(self, params, grad, ms, mom, lr_dev, decay, momentum, eps, clip_norm, clip_mode, grad_scale=1.0,
                     gnorm_out=None):
        self._clip_step("paac_clip_rmsprop", params, grad, (("ms", ms), ("mom", mom)), (), lr_dev, (decay, momentum, eps),
                        clip_norm, clip_mode, grad_scale, gnorm_out)

    def clip_adam(self, params, grad, m, v, beta_powers, lr_dev, beta1, beta2, eps, clip_norm, clip_mode, grad_scale=1.0,
                  gnorm_out=None):
        """The same clipped gradient through TF Adam instead of RMSProp (include/paac_hip.h: paac_clip_adam); beta_powers is
        the device float32[2] {beta1_power, beta2_power} the step reads and advances."""
        self._clip_step("paac_clip_adam", params, grad, (("m", m), ("v", v)),
                        (_ptr(beta_powers, torch.float32, 2, "beta_powers"),), lr_dev, (beta1, beta2, eps), clip_norm,
                        clip_mode, grad_scale, gnorm_out)

    @staticmethod
    def _kl_gate(kl, scale, thr, first, stop, applied, checked):
        """-> _lib.KlGate (include/paac_hip.h: paac_kl_gate).  kl: float32 tensor whose first element is the statistic; stop:
        int32[1]; applied (int32) / checked (float32): one-element views or None.  A kl / stop of None goes through as NULL
        (the entry refuses it)."""
        return _lib.KlGate(_ptr(kl, torch.float32, 1, "gate kl", True), float(scale), float(thr), 1 if first else 0,
                           _ptr(stop, torch.int32, 1, "gate stop", True), _ptr(applied, torch.int32, 1, "gate applied", True),
                           _ptr(checked, torch.float32, 1, "gate checked", True))

    def clip_rmsprop_gated(self, params, grad, ms, mom, lr_dev, decay, momentum, eps, clip_norm, clip_mode, grad_scale=1.0,
                           gnorm_out=None, *, kl, thr, first, stop, applied=None, checked=None, kl_scale=1.0):
        """clip_rmsprop behind a --ppo_target_kl gate (include/paac_hip.h: paac_clip_rmsprop_gated): the step is skipped, and
        *stop set, unless kl[0] * kl_scale <= thr and *stop was clear (first clears it before the comparison)."""
        self._clip_step("paac_clip_rmsprop_gated", params, grad, (("ms", ms), ("mom", mom)), (), lr_dev,
                        (decay, momentum, eps), clip_norm, clip_mode, grad_scale, gnorm_out,
                        self._kl_gate(kl, kl_scale, thr, first, stop, applied, checked))

    def clip_adam_gated(self, params, grad, m, v, beta_powers, lr_dev, beta1, beta2, eps, clip_norm, clip_mode, grad_scale=1.0,
                        gnorm_out=None, *, kl, thr, first, stop, applied=None, checked=None, kl_scale=1.0):
        """clip_adam behind a --ppo_target_kl gate (include/paac_hip.h: paac_clip_adam_gated); a skipped step leaves the powers."""
        self._clip_step("paac_clip_adam_gated", params, grad, (("m", m), ("v", v)),
                        (_ptr(beta_powers, torch.float32, 2, "beta_powers"),), lr_dev, (beta1, beta2, eps), clip_norm,
                        clip_mode, grad_scale, gnorm_out,
                        self._kl_gate(kl, kl_scale, thr, first, stop, applied, checked))

    def keep_next_forward(self, train_row):
        """The next acting forward also leaves its rows' activations at rows [train_row, train_row + batch) of the training
        activation set (include/paac_hip.h: paac_keep_next_forward); -1 cancels."""
        _lib.check(self.lib.paac_keep_next_forward(self.handle, int(train_row)), "paac_keep_next_forward")

    def bootstrap_forward_trunk(self, params, states, train_row):
        """Acting-shaped forward (conv tower + fc) of the bootstrap observations, kept at rows [train_row, ...) of the training
        set the acting steps have filled: the next loss_backward[_returns](forward_done=True) needs no training forward."""
        B = self._check_states(states)
        _lib.check(self.lib.paac_bootstrap_forward_trunk(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                                         _ptr(states, torch.uint8, B * 28224, "states"), B, int(train_row), _stream()),
                   "paac_bootstrap_forward_trunk")

    def act_step_mt(self, params, states, mt_state, actions, probs_out, values_out, env_seed, env_offset,
                    terminal_threshold, step_base_dev, step_offset, stack_out, rewards_out, masks_out, ep_reward, ep_len,
                    finished=None, stack_out2=None, raw_scratch=None, walk_scratch=None):
        """One acting step in three launches: policy forward, then heads finish + numpy-parity sampler + synthetic
        environment step in one (include/paac_hip.h: paac_act_step_mt).  raw_scratch ([N,2,210,160] u8): path B -- the
        step launch writes the raw screen pairs, a fourth launch (max, PIL-nearest resize, history push) builds the stacks."""
        N, A = self._check_states(states), self.num_actions
        if N > ACT_STEP_MAX_ENVS_LARGE or N * (A - 1) > FUSED_SAMPLE_MAX_DRAWS:
            raise ValueError("act_step_mt supports N <= %d and N*(A-1) <= %d" % (ACT_STEP_MAX_ENVS_LARGE, FUSED_SAMPLE_MAX_DRAWS))
        if stack_out is None:
            raise ValueError("stack_out is required")
        step = _step_ptrs(N, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, states=states)
        self._act(N, params, states, mt_state, actions, probs_out, values_out, step, env_seed, env_offset, terminal_threshold,
                  step_base_dev, step_offset, raw_scratch, walk_scratch)

    def act_step_pipe(self, params, states, mt_state, actions, probs_out, values_out, env_seed, env_offset,
                      terminal_threshold, step_base_dev, step_offset, stack_out, rewards_out, masks_out, ep_reward, ep_len,
                      finished=None, stack_out2=None):
        """act_step_mt with the sampler off the dependent chain, two launches per step (include/paac_hip.h:
        paac_act_step_pipe): conv tower, then the fc launch, which also shifts this step's frames and finishes, samples and
        records the PREVIOUS pipelined step.  This step's actions, probabilities, values and records are owed until the next
        act_step_pipe, bootstrap_forward_trunk or act_step_flush.  Path A, N <= ACT_STEP_MAX_ENVS, N*(A-1) <= 1024."""
        N = self._check_states(states)
        if stack_out is None:
            raise ValueError("stack_out is required")
        step = _step_ptrs(N, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, states=states)
        self._act(N, params, states, mt_state, actions, probs_out, values_out, step, env_seed, env_offset, terminal_threshold,
                  step_base_dev, step_offset, entry="paac_act_step_pipe")

    def act_step_flush(self):
        """Pay the sample the last act_step_pipe owes, as a launch of its own; nothing pending: nothing launched."""
        _lib.check(self.lib.paac_act_step_flush(self.handle, _stream()), "paac_act_step_flush")

    def act_step_pending(self):
        """True while the last act_step_pipe's sample is owed (host-side state of the context)."""
        return bool(self.lib.paac_act_step_pending(self.handle))

    def act_mt(self, params, states, mt_state, actions, probs_out, values_out):
        """Policy forward + numpy-parity sampler in three launches, no environment step (paac_act_step_mt with stack_out =
        NULL): what the host-plugin loop runs per step (paac.py:104-110).  N <= ACT_STEP_MAX_ENVS, N*(A-1) <= 1024."""
        N = self._check_states(states)
        self._act(N, params, states, mt_state, actions, probs_out, values_out, _step_ptrs(N))

    def _act(self, N, params, states, mt_state, actions, probs_out, values_out, step, env_seed=0, env_offset=0,
             terminal_threshold=0, step_base_dev=None, step_offset=0, raw_scratch=None, walk_scratch=None,
             entry="paac_act_step_mt"):
        """paac_act_step_mt (or paac_act_step_pipe: the same arguments); step: _step_ptrs' list."""
        A = self.num_actions
        _lib.check(getattr(self.lib, entry)(
            self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
            _ptr(states, torch.uint8, N * 28224, "states"), N, _ptr(mt_state, torch.int32, 625, "mt_state"),
            _ptr(actions, torch.int32, N, "actions"), _ptr(probs_out, torch.float32, N * A, "probs_out"),
            _ptr(values_out, torch.float32, N, "values_out"), int(env_seed), int(env_offset), int(terminal_threshold),
            _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset), *step,
            _ptr(raw_scratch, torch.uint8, N * 2 * RAW_H * RAW_W, "raw_scratch", True),
            *_lent(walk_scratch), _stream()), entry)

    def pack_weights(self, params):
        """Refresh the ctx's pre-split copy of the conv weights (include/paac_hip.h: paac_pack_weights)."""
        _lib.check(self.lib.paac_pack_weights(self.handle, _ptr(params, torch.float32, self.layout["total"], "params"),
                                              _stream()), "paac_pack_weights")

    def set_managed_weights(self, on=True):
        """Managed mode: only clip_rmsprop / pack_weights refresh the pre-split copy; acting forwards keep no conv1 /
        conv2 activations (include/paac_hip.h: paac_set_managed_weights)."""
        _lib.check(self.lib.paac_set_managed_weights(self.handle, 1 if on else 0), "paac_set_managed_weights")

    def grad_stats(self, clip_norm, clip_mode):
        """Gradient summaries of the last clip_rmsprop (actor_learner.py:85-87, logger_utils.py:23-33): dict with
        mean / stddev / max / min of the raw and of the clipped flat gradient, and global_norm (of the raw gradient,
        or of the clipped one in local mode, as the reference's global_norm tensor holds).  Local mode adds "tensors":
        {name: {"norm": raw L2 norm, "factor": factor applied}}.  Synchronises."""
        out = torch.zeros(8, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.paac_grad_stats(self.handle, ctypes.c_void_p(out.data_ptr()), _stream()), "paac_grad_stats")
        s, ss, mx, mn = [float(v) for v in out.cpu().numpy()[:4].astype(np.float64)]
        n = float(self.layout["total_unpadded"])
        mean = s / n
        std = max(ss / n - mean * mean, 0.0) ** 0.5
        gn = ss ** 0.5
        raw = {"mean": mean, "stddev": std, "max": mx, "min": mn}
        if clip_mode == _lib.CLIP_LOCAL:
            # the clipped gradient is tensor i's raw one times f_i: its summaries are folded from the per-tensor ones
            ts = self.grad_tensor_stats()
            f = ts[:, 5]
            cs, css = float(np.sum(f * ts[:, 0])), float(np.sum(f * f * ts[:, 1]))
            cmean = cs / n
            return {"global_norm": css ** 0.5, "raw_gradients": raw,
                    "clipped_gradients": {"mean": cmean, "stddev": max(css / n - cmean * cmean, 0.0) ** 0.5,
                                          "max": float(np.max(f * ts[:, 2])), "min": float(np.min(f * ts[:, 3]))},
                    "tensors": {t["name"]: {"norm": float(ts[i, 1]) ** 0.5, "factor": float(f[i])}
                                for i, t in enumerate(self.layout["tensors"])}}
        f = 1.0
        if clip_mode == _lib.CLIP_GLOBAL and gn > 0.0:
            f = clip_norm * min(1.0 / gn, 1.0 / clip_norm)
        return {"global_norm": gn,
                "raw_gradients": raw,
                "clipped_gradients": {"mean": mean * f, "stddev": std * f, "max": mx * f, "min": mn * f}}

    def grad_tensor_stats(self):
        """Per-tensor summaries of the last clip_rmsprop, which must have run in local mode (include/paac_hip.h:
        paac_grad_tensor_stats): float64 array [num_tensors, 8], row i = {sum, sum of squares, max, min, real zeros,
        factor applied, 0, 0} of tensor i's raw gradient.  Synchronises."""
        out = torch.zeros(_lib.MAX_TENSORS * 8, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.paac_grad_tensor_stats(self.handle, ctypes.c_void_p(out.data_ptr()), _stream()),
                   "paac_grad_tensor_stats")
        return out.cpu().numpy().astype(np.float64).reshape(_lib.MAX_TENSORS, 8)[:len(self.layout["tensors"])]

    def debug_activation(self, what, batch):
        convs, fc = arch_geometry(self.arch)
        cap = int(batch) * self.num_actions if int(what) == 26 else activation_size(convs, fc, what, batch)
        if cap is None:
            raise ValueError("debug_activation: what=%d is not an activation of this geometry" % what)
        out = torch.empty(cap, dtype=torch.float32, device=self.device)
        n = self.lib.paac_debug_activation(self.handle, int(what), int(batch), ctypes.c_void_p(out.data_ptr()), cap, _stream())
        _lib.check(n, "paac_debug_activation")
        return out[:n].clone()

    # -- timing hooks ----------------------------------------------------------------------------
    def prof_enable(self, on=True):
        _lib.check(self.lib.paac_prof_enable(self.handle, 1 if on else 0), "paac_prof_enable")

    def prof_read(self, with_mix=False):
        """-> list of (family name, batch, milliseconds), one per kernel-family launch since the last read; with_mix adds
        the launch's instruction mix as a tuple of MFMA products per fp32 multiply, one entry per contraction body
        (include/paac_hip.h: paac_prof_read_mix)."""
        cap = 8192
        fam = (ctypes.c_int32 * cap)()
        bat = (ctypes.c_int32 * cap)()
        ms = (ctypes.c_float * cap)()
        mix = (ctypes.c_int32 * cap)()
        if with_mix:
            _lib.check(self.lib.paac_prof_read_mix(self.handle, mix, cap), "paac_prof_read_mix")
        n = self.lib.paac_prof_read(self.handle, fam, bat, ms, cap)
        _lib.check(n, "paac_prof_read")
        out = [(self.lib.paac_prof_name(fam[i]).decode(), int(bat[i]), float(ms[i])) for i in range(n)]
        if with_mix:
            out = [o + (tuple(b for b in ((mix[i] >> (8 * k)) & 255 for k in range(4)) if b),) for i, o in enumerate(out)]
        return out


# -- context-free entry points -------------------------------------------------------------------
def lr_step(global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev):
    lib = _lib.load()
    _lib.check(lib.paac_lr_step(_ptr(global_step_dev, torch.int64, 1, "global_step"), int(increment), float(initial_lr),
                                int(lr_annealing_steps), _ptr(lr_out_dev, torch.float32, 1, "lr_out"), _stream()),
               "paac_lr_step")


def _returns_struct(v_boot, rewards, masks, values, gamma, y_out, adv_out, global_step_dev, increment, initial_lr,
                    lr_annealing_steps, lr_out_dev, tick_dev, tick_inc, gae_lambda, truncs=None):
    T, N = rewards.shape
    if truncs is not None and tuple(truncs.shape) != (T, N):
        raise ValueError("truncs must be [%d,%d] like the rewards, got %s" % (T, N, tuple(truncs.shape)))
    fields = dict(
        v_boot=_ptr(v_boot, torch.float32, N, "v_boot", True), rewards=_ptr(rewards, torch.float32, T * N, "rewards"),
        masks=_ptr(masks, torch.float32, T * N, "masks"), values=_ptr(values, torch.float32, T * N, "values"), T=T, N=N,
        gamma=float(gamma), y_out=_ptr(y_out, torch.float32, T * N, "y_out"), adv_out=_ptr(adv_out, torch.float32, T * N, "adv_out"),
        global_step_dev=_ptr(global_step_dev, torch.int64, 1, "global_step", True), increment=int(increment),
        initial_lr=float(initial_lr), lr_annealing_steps=int(lr_annealing_steps),
        lr_out_dev=_ptr(lr_out_dev, torch.float32, 1, "lr_out", True),
        tick_dev=_ptr(tick_dev, torch.int64, 1, "tick", True), tick_inc=int(tick_inc),
        estimator=_lib.RETURNS_GAE if uses_gae(gae_lambda) else _lib.RETURNS_NSTEP,
        gae_lambda=float(gae_lambda) if uses_gae(gae_lambda) else 0.0)
    if truncs is None:
        return _lib.Returns(**fields)
    # the plane travels behind the block (include/paac_hip.h: paac_returns_truncs): the entries get the `ret` member, which
    # keeps the whole record alive
    fields["estimator"] |= _lib.RETURNS_TRUNCS
    return _lib.ReturnsTruncs(_lib.Returns(**fields), _ptr(truncs, torch.float32, T * N, "truncs")).ret


def adv_normalize(adv, adv_n_out, stats_out=None):
    """--adv_norm's normalisation on its own (include/paac_hip.h: paac_adv_normalize): adv_n_out = (adv - mean) / (std + 1e-8)
    over all of adv, fp64 statistics in a fixed order.  stats_out: float64[2] = {mean, std}."""
    B = adv.numel()
    lib = _lib.load()
    _lib.check(lib.paac_adv_normalize(_ptr(adv, torch.float32, B, "adv"), B, _ptr(adv_n_out, torch.float32, B, "adv_n_out"),
                                      _ptr(stats_out, torch.float64, 2, "stats_out", True), _stream()), "paac_adv_normalize")


def returns_norm_tick(v_boot, rewards, masks, values, gamma, y_out, adv_out, adv_n_out, stats_out=None, global_step_dev=None,
                      increment=0, initial_lr=0.0, lr_annealing_steps=1, lr_out_dev=None, tick_dev=None, tick_inc=0,
                      gae_lambda=None, truncs=None):
    """paac_returns_norm_tick with the bootstrap values given (no ctx): == nstep_returns_tick / gae_returns_tick followed by
    adv_normalize, in one launch.  truncs: the truncation plane of --bootstrap_truncated, None = off."""
    T, N = rewards.shape
    ret = _returns_struct(v_boot, rewards, masks, values, gamma, y_out, adv_out, global_step_dev, increment, initial_lr,
                          lr_annealing_steps, lr_out_dev, tick_dev, tick_inc, gae_lambda, truncs)
    if not ret.v_boot:
        raise ValueError("returns_norm_tick: v_boot is required without a ctx (Context.returns_norm_tick takes it from the "
                         "training forward)")
    lib = _lib.load()
    _lib.check(lib.paac_returns_norm_tick(None, None, ctypes.byref(ret), _ptr(adv_n_out, torch.float32, T * N, "adv_n_out"),
                                          _ptr(stats_out, torch.float64, 2, "stats_out", True), _stream()),
               "paac_returns_norm_tick")


def window_fields():
    """-> (n_f, n_i): the lengths of the --window_stats block the library was compiled for."""
    n_f, n_i = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().paac_window_fields(ctypes.byref(n_f), ctypes.byref(n_i)), "paac_window_fields")
    return int(n_f.value), int(n_i.value)


def window_block(device):
    """An empty --window_stats block on `device`: (acc_f float64[N_F], acc_i int64[N_I]), the spec's tables checked against
    the compiled layout."""
    from . import window_stats
    if window_fields() != (window_stats.N_F, window_stats.N_I):
        raise _lib.PaacHipError("window_stats.FIELDS_F / FIELDS_I hold %d / %d fields, the library was compiled for %d / %d"
                                % ((window_stats.N_F, window_stats.N_I) + window_fields()))
    return (torch.zeros(window_stats.N_F, dtype=torch.float64, device=device),
            torch.zeros(window_stats.N_I, dtype=torch.int64, device=device))


def window_fold(acc_f, acc_i, values, rewards, masks, actions, y, adv, num_actions, loss, gnorm, truncs=None, loss0=None,
                ppo_stats=None, stats_first=0, applied=None, finished=None):
    """--window_stats: one cycle folded into the block (include/paac_hip.h: paac_window_fold; spec: paac_amd/window_stats.py).
    values / rewards / masks / actions (and truncs, or None) [T, N]; y / adv [T*N]; loss [steps, 4] (loss0 [4]: in place of its
    row 0); ppo_stats [steps, 2 or 3] or None; applied int32 [steps] or None; gnorm [1]; finished: the episode ring or None."""
    from . import window_stats
    if values.dim() != 2:
        raise ValueError("values must be [T,N], got %s" % (tuple(values.shape),))
    T, N = values.shape
    for nm, t in (("rewards", rewards), ("masks", masks), ("actions", actions), ("truncs", truncs)):
        if t is not None and tuple(t.shape) != (T, N):
            raise ValueError("%s must be [%d,%d] like the values, got %s" % (nm, T, N, tuple(t.shape)))
    if loss.dim() != 2 or loss.shape[1] != 4:
        raise ValueError("loss must be [steps,4], got %s" % (tuple(loss.shape),))
    steps = loss.shape[0]
    cols = 0
    if ppo_stats is not None:
        if ppo_stats.dim() != 2 or ppo_stats.shape[0] != steps or ppo_stats.shape[1] not in (2, 3):
            raise ValueError("ppo_stats must be [%d,2] or [%d,3], got %s" % (steps, steps, tuple(ppo_stats.shape)))
        cols = ppo_stats.shape[1]
    if finished is not None and finished.numel() * finished.element_size() < FINISHED_RING_BYTES:
        raise ValueError("finished ring too small")
    f32 = torch.float32
    block = _lib.WindowInputs(
        T, N, int(num_actions), _ptr(values, f32, T * N, "values"), _ptr(rewards, f32, T * N, "rewards"),
        _ptr(masks, f32, T * N, "masks"), _ptr(actions, torch.int32, T * N, "actions"), _ptr(y, f32, T * N, "y"),
        _ptr(adv, f32, T * N, "adv"), _ptr(truncs, f32, T * N, "truncs", True), _ptr(loss, f32, steps * 4, "loss"),
        _ptr(loss0, f32, 4, "loss0", True), steps, _ptr(ppo_stats, f32, steps * cols, "ppo_stats", True), cols, int(stats_first),
        _ptr(applied, torch.int32, steps, "applied", True), _ptr(gnorm, f32, 1, "gnorm"),
        _ptr(finished, torch.int32, FINISHED_RING_BYTES // 4, "finished", True))
    _lib.check(_lib.load().paac_window_fold(ctypes.byref(block), _ptr(acc_f, torch.float64, window_stats.N_F, "acc_f"),
                                            _ptr(acc_i, torch.int64, window_stats.N_I, "acc_i"), _stream()), "paac_window_fold")


def uses_gae(gae_lambda):
    """THE routing rule of --gae_lambda: None (not given) and exactly 1.0 mean the reference's n-step return through the
    n-step kernels -- GAE(1) is the same quantity only up to the last place -- and every other value the GAE kernels."""
    return gae_lambda is not None and float(gae_lambda) != 1.0


def returns_scan(v_boot, rewards, masks, values, gamma, y, adv, gae_lambda=None, truncs=None, global_step_dev=None, increment=0,
                 initial_lr=0.0, lr_annealing_steps=1, lr_out_dev=None, tick_dev=None, tick_inc=0, estimator=None):
    """The standalone scan from the argument block (include/paac_hip.h: paac_returns_scan): the estimator by the routing rule
    (uses_gae), the _tick entries' bookkeeping when global_step_dev is given, and the truncation plane of
    --bootstrap_truncated (float32[T,N]; None runs the plain kernels).  estimator="gae": GAE whatever the rule says (GAE(1),
    which gae_returns also accepts)."""
    if v_boot is None:
        raise ValueError("returns_scan: v_boot is required")
    ret = _returns_struct(v_boot, rewards, masks, values, gamma, y, adv, global_step_dev, increment, initial_lr,
                          lr_annealing_steps, lr_out_dev, tick_dev, tick_inc, gae_lambda, truncs)
    if estimator == "gae":
        ret.estimator = (ret.estimator & _lib.RETURNS_TRUNCS) | _lib.RETURNS_GAE
        ret.gae_lambda = float(gae_lambda)
    elif estimator is not None:
        raise ValueError("returns_scan: estimator %r (None or 'gae')" % (estimator,))
    _lib.check(_lib.load().paac_returns_scan(ctypes.byref(ret), _stream()), "paac_returns_scan")


def returns(v_boot, rewards, masks, values, gamma, y, adv, gae_lambda=None, truncs=None):
    """nstep_returns or gae_returns by the routing rule (uses_gae); with a truncation plane, returns_scan."""
    if truncs is not None:
        returns_scan(v_boot, rewards, masks, values, gamma, y, adv, gae_lambda, truncs)
    elif uses_gae(gae_lambda):
        gae_returns(v_boot, rewards, masks, values, gamma, gae_lambda, y, adv)
    else:
        nstep_returns(v_boot, rewards, masks, values, gamma, y, adv)


def returns_tick(v_boot, rewards, masks, values, gamma, y, adv, gae_lambda=None, truncs=None, **tick):
    """nstep_returns_tick or gae_returns_tick by the same rule; tick: their bookkeeping keyword arguments."""
    if truncs is not None:
        returns_scan(v_boot, rewards, masks, values, gamma, y, adv, gae_lambda, truncs, **tick)
    elif uses_gae(gae_lambda):
        gae_returns_tick(v_boot, rewards, masks, values, gamma, gae_lambda, y, adv, **tick)
    else:
        nstep_returns_tick(v_boot, rewards, masks, values, gamma, y, adv, **tick)


def _returns_scan(name, v_boot, rewards, masks, values, gamma, lam, y, adv, tick=None):
    """The four standalone entries (include/paac_hip.h).  lam: (gae_lambda,) from the GAE pair, () from the n-step pair;
    tick: (global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc) from the _tick pair."""
    T, N = rewards.shape
    args = [_ptr(v_boot, torch.float32, N, "v_boot"), _ptr(rewards, torch.float32, T * N, "rewards"),
            _ptr(masks, torch.float32, T * N, "masks"), _ptr(values, torch.float32, T * N, "values"), T, N, float(gamma),
            *lam, _ptr(y, torch.float32, T * N, "y"), _ptr(adv, torch.float32, T * N, "adv")]
    if tick is not None:
        global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc = tick
        args += [_ptr(global_step_dev, torch.int64, 1, "global_step"), int(increment), float(initial_lr),
                 int(lr_annealing_steps), _ptr(lr_out_dev, torch.float32, 1, "lr_out"),
                 _ptr(tick_dev, torch.int64, 1, "tick", True), int(tick_inc)]
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def gae_returns(v_boot, rewards, masks, values, gamma, gae_lambda, y, adv):
    """Generalized advantage estimation on the rollout records (include/paac_hip.h: paac_gae_returns)."""
    _returns_scan("paac_gae_returns", v_boot, rewards, masks, values, gamma, (float(gae_lambda),), y, adv)


def gae_returns_tick(v_boot, rewards, masks, values, gamma, gae_lambda, y, adv, global_step_dev, increment, initial_lr,
                     lr_annealing_steps, lr_out_dev, tick_dev=None, tick_inc=0):
    _returns_scan("paac_gae_returns_tick", v_boot, rewards, masks, values, gamma, (float(gae_lambda),), y, adv,
                  (global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc))


def nstep_returns(v_boot, rewards, masks, values, gamma, y, adv):
    _returns_scan("paac_nstep_returns", v_boot, rewards, masks, values, gamma, (), y, adv)


def nstep_returns_tick(v_boot, rewards, masks, values, gamma, y, adv, global_step_dev, increment, initial_lr,
                       lr_annealing_steps, lr_out_dev, tick_dev=None, tick_inc=0):
    _returns_scan("paac_nstep_returns_tick", v_boot, rewards, masks, values, gamma, (), y, adv,
                  (global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc))


def sample_mt_scratch(N, A, device):
    nbytes = _lib.load().paac_sample_mt_scratch_bytes(int(N), int(A))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def sample_mt(probs, mt_state, scratch, actions):
    N, A = probs.shape
    lib = _lib.load()
    need = lib.paac_sample_mt_scratch_bytes(int(N), int(A))
    if scratch.numel() * scratch.element_size() < need:
        raise ValueError("sample_mt scratch too small: %d < %d bytes" % (scratch.numel() * scratch.element_size(), need))
    _lib.check(lib.paac_sample_mt(_ptr(probs, torch.float32, N * A, "probs"), N, A,
                                  _ptr(mt_state, torch.int32, 625, "mt_state"), ctypes.c_void_p(scratch.data_ptr()),
                                  _ptr(actions, torch.int32, N, "actions"), _stream()), "paac_sample_mt")


def mt_state_from_numpy(state, device):
    """np.random.get_state() tuple -> device int32[625] (key + pos)."""
    assert state[0] == "MT19937"
    arr = np.concatenate([np.asarray(state[1], dtype=np.uint32), np.array([state[2]], dtype=np.uint32)])
    return torch.from_numpy(arr.view(np.int32).copy()).to(device)


def mt_state_to_numpy(mt_state):
    arr = mt_state.detach().cpu().numpy().view(np.uint32)
    return ("MT19937", arr[:624].copy(), int(arr[624]), 0, 0.0)


def sample_philox(probs, seed, step_base_dev, step_offset, env_offset, actions):
    N, A = probs.shape
    lib = _lib.load()
    _lib.check(lib.paac_sample_philox(_ptr(probs, torch.float32, N * A, "probs"), N, A, int(seed),
                                      _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset),
                                      int(env_offset), _ptr(actions, torch.int32, N, "actions"), _stream()),
               "paac_sample_philox")


def minibatch_perms(B, seed, step_base_dev, step_offset, perms_out):
    """perms_out int32 [K, B]: row e = epoch e's shuffle of 0..B-1 (include/paac_hip.h: paac_minibatch_perms), the stable argsort
    of philox4x32-10 keys on counter (row, step lo, step hi, 0x504D0000 + e), step = *step_base_dev + step_offset."""
    B = int(B)
    if perms_out.dim() != 2 or perms_out.shape[1] != B:
        raise ValueError("perms_out must be int32 [epochs, %d], got %s" % (B, tuple(perms_out.shape)))
    K = int(perms_out.shape[0])
    if not 1 <= B <= _lib.MINIBATCH_MAX_ROWS or not 1 <= K <= _lib.PPO_EPOCHS_MAX:
        raise ValueError("minibatch_perms: B=%d (1..%d), epochs=%d (1..%d)" % (B, _lib.MINIBATCH_MAX_ROWS, K, _lib.PPO_EPOCHS_MAX))
    _lib.check(_lib.load().paac_minibatch_perms(B, K, int(seed), _ptr(step_base_dev, torch.int64, 1, "step_base", True),
                                                int(step_offset), _ptr(perms_out, torch.int32, K * B, "perms_out"), _stream()),
               "paac_minibatch_perms")


def gather_minibatch(perm, states=None, states_out=None, actions=None, actions_out=None, y=None, y_out=None, adv=None,
                     adv_out=None, p_old=None, p_old_out=None, v_old=None, v_old_out=None):
    """out[r] = in[perm[r]] for the states ([B,84,84,4] u8, 16-byte vectors) and the small [B] arrays in one launch
    (include/paac_hip.h: paac_gather_minibatch).  Every array comes with its output or not at all; an output that overlaps its
    input is refused."""
    B = int(perm.numel())
    if not 1 <= B <= _lib.MINIBATCH_MAX_ROWS:
        raise ValueError("gather_minibatch: %d rows outside [1, %d]" % (B, _lib.MINIBATCH_MAX_ROWS))
    pairs = (("states", states, states_out, torch.uint8, B * 28224), ("actions", actions, actions_out, torch.int32, B),
             ("y", y, y_out, torch.float32, B), ("adv", adv, adv_out, torch.float32, B),
             ("p_old", p_old, p_old_out, torch.float32, B), ("v_old", v_old, v_old_out, torch.float32, B))
    ptrs = []
    for name, src, dst, dtype, numel in pairs:
        if (src is None) != (dst is None):
            raise ValueError("gather_minibatch: %s and %s_out must both be given or both be None" % (name, name))
        if src is not None:
            a, b, nbytes = src.data_ptr(), dst.data_ptr(), numel * src.element_size()
            if a < b + nbytes and b < a + nbytes:
                raise ValueError("gather_minibatch: %s_out overlaps %s (the gather cannot run in place)" % (name, name))
        ptrs += [_ptr(src, dtype, numel, name, True), _ptr(dst, dtype, numel, name + "_out", True)]
    if states is not None and tuple(states.shape[1:]) != OBS_SHAPE:
        raise ValueError("states must be [B,84,84,4] uint8, got %s" % (tuple(states.shape),))
    _lib.check(_lib.load().paac_gather_minibatch(_ptr(perm, torch.int32, B, "perm"), B, *(ptrs + [_stream()])),
               "paac_gather_minibatch")


def debug_clock(out2_dev):
    _lib.check(_lib.load().paac_debug_clock(_ptr(out2_dev, torch.int64, 2, "out2"), _stream()), "paac_debug_clock")


def counter_add(counter_dev, inc):
    _lib.check(_lib.load().paac_counter_add(_ptr(counter_dev, torch.int64, 1, "counter"), int(inc), _stream()),
               "paac_counter_add")


def preprocess_stack(raw, stack_in, stack_out, push_mask=None, reset_mask=None):
    N = raw.shape[0]
    if tuple(raw.shape) == (N, 2, RAW_H, RAW_W):
        rgb = 0
    elif tuple(raw.shape) == (N, 2, RAW_H, RAW_W, 3):
        rgb = 1
    else:
        raise ValueError("raw must be [N,2,210,160] or [N,2,210,160,3] uint8, got %s" % (tuple(raw.shape),))
    for nm, t in (("stack_in", stack_in), ("stack_out", stack_out)):
        if tuple(t.shape) != (N,) + OBS_SHAPE:
            raise ValueError("%s must be [%d,84,84,4], got %s" % (nm, N, tuple(t.shape)))
    _lib.check(_lib.load().paac_preprocess_stack(_ptr(raw, torch.uint8, None, "raw"), rgb, N,
                                                 _ptr(stack_in, torch.uint8, N * 28224, "stack_in"),
                                                 _ptr(stack_out, torch.uint8, N * 28224, "stack_out"),
                                                 _ptr(push_mask, torch.uint8, N, "push_mask", True),
                                                 _ptr(reset_mask, torch.uint8, N, "reset_mask", True), _stream()),
               "paac_preprocess_stack")


def synth_reset(seed, env_offset, stack_out, raw_scratch=None):
    N = stack_out.shape[0]
    if tuple(stack_out.shape) != (N,) + OBS_SHAPE:
        raise ValueError("stack_out must be [N,84,84,4]")
    _lib.check(_lib.load().paac_synth_reset(int(seed), int(env_offset), N, _ptr(stack_out, torch.uint8, N * 28224, "stack_out"),
                                            _ptr(raw_scratch, torch.uint8, N * 2 * RAW_H * RAW_W, "raw_scratch", True),
                                            _stream()), "paac_synth_reset")


def synth_step(seed, env_offset, actions, terminal_threshold, step_base_dev, step_offset, stack_in, stack_out,
               rewards_out, masks_out, ep_reward, ep_len, finished=None, stack_out2=None, raw_scratch=None):
    N = actions.shape[0]
    step = _step_ptrs(N, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, stack_in=stack_in)
    _lib.check(_lib.load().paac_synth_step(int(seed), int(env_offset), N, _ptr(actions, torch.int32, N, "actions"),
                                           int(terminal_threshold), _ptr(step_base_dev, torch.int64, 1, "step_base", True),
                                           int(step_offset), _ptr(stack_in, torch.uint8, N * 28224, "stack_in"), *step,
                                           _ptr(raw_scratch, torch.uint8, N * 2 * RAW_H * RAW_W, "raw_scratch", True),
                                           _stream()), "paac_synth_step")


# The device games that carry a state record (csrc/<game>_dev.h): int32 words of a record (paac_amd/<game>.py: STATE_WORDS),
# the id paac_eval_step knows the game by, and the keyword of the step's one integer option, which follows `finished` in
# paac_<game>_step (None: the game has none).  The entry points are paac_<game>_reset / paac_<game>_step.
DEVICE_GAMES = {
    "catch": dict(words=8, eval_id=_lib.EVAL_CATCH, step_option=None),
    "bricks": dict(words=12, eval_id=_lib.EVAL_BRICKS, step_option="single_life"),
    "rally": dict(words=12, eval_id=_lib.EVAL_RALLY, step_option=None),
}


def _stateful_reset(entry, words, seed, env_offset, state_out, stack_out):
    """paac_<game>_reset of a game whose environments carry a state record of `words` int32."""
    N = stack_out.shape[0]
    if tuple(stack_out.shape) != (N,) + OBS_SHAPE:
        raise ValueError("stack_out must be [N,84,84,4]")
    _lib.check(getattr(_lib.load(), entry)(int(seed), int(env_offset), N, *_state_ptrs(N, words, state_out=state_out),
                                           _ptr(stack_out, torch.uint8, N * 28224, "stack_out"), _stream()), entry)


def _stateful_step(entry, words, seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out,
                   ep_reward, ep_len, finished, stack_out2, state_out2, extra=()):
    """paac_<game>_step: the shape checks and the argument list the stateful games share; `extra` = the game's own integer
    arguments, which follow `finished`."""
    N, buffers, records = _game_step_ptrs(words, actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2,
                                          rewards_out, masks_out, ep_reward, ep_len, finished)
    _lib.check(getattr(_lib.load(), entry)(int(seed), int(env_offset), N, *buffers, *records, *(int(x) for x in extra), _stream()),
               entry)


def game_reset(kind, seed, env_offset, state_out, stack_out):
    _stateful_reset("paac_%s_reset" % kind, DEVICE_GAMES[kind]["words"], seed, env_offset, state_out, stack_out)


def game_step_records(kind, seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out, ep_reward,
                      ep_len, finished=None, stack_out2=None, state_out2=None, truncs_out=None, **option):
    """paac_game_step (include/paac_hip.h): game_step by the game's id with the records as one block, truncs_out float32[N]
    (--bootstrap_truncated: 1 where the step ended its episode at the step cap alone; None: not written) among them."""
    game = DEVICE_GAMES[kind]
    name, words = game["step_option"], game["words"]
    if set(option) - {name}:
        raise TypeError("%s_step: unexpected keyword arguments %s" % (kind, sorted(set(option) - {name})))
    N, buffers, records = _game_step_ptrs(words, actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2,
                                          rewards_out, masks_out, ep_reward, ep_len, finished)
    rec = _env_records(N, records, truncs_out)
    _lib.check(_lib.load().paac_game_step(game["eval_id"], int(seed), int(env_offset), N, *buffers, ctypes.byref(rec),
                                          int(bool(option.get(name, False))) if name else 0, _stream()), "paac_game_step")


def game_step(kind, seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out, ep_reward, ep_len,
              finished=None, stack_out2=None, state_out2=None, truncs_out=None, **option):
    """`option`: the game's step option by its keyword (DEVICE_GAMES: bricks' single_life, False if not given).  truncs_out: the
    step goes through game_step_records, which writes the truncation plane; None is the game's own entry, as always."""
    if truncs_out is not None:
        return game_step_records(kind, seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out,
                                 ep_reward, ep_len, finished, stack_out2, state_out2, truncs_out, **option)
    game = DEVICE_GAMES[kind]
    name = game["step_option"]
    if set(option) - {name}:
        raise TypeError("%s_step: unexpected keyword arguments %s" % (kind, sorted(set(option) - {name})))
    extra = (bool(option.get(name, False)),) if name else ()
    _stateful_step("paac_%s_step" % kind, game["words"], seed, env_offset, actions, state_in, state_out, stack_in, stack_out,
                   rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, state_out2, extra=extra)


# the games by name: catch_reset / catch_step / CATCH_STATE_WORDS, and the same for bricks and rally
for _kind, _game in DEVICE_GAMES.items():
    globals().update({_kind + "_reset": functools.partial(game_reset, _kind), _kind + "_step": functools.partial(game_step, _kind),
                      _kind.upper() + "_STATE_WORDS": _game["words"]})
EVAL_GAMES = {kind: (game["eval_id"], game["words"]) for kind, game in DEVICE_GAMES.items()}

# The paired games (csrc/game_dev.h): N rows = N / 2 boards, a row's step reads its partner's action too.  A table of their
# own: they have no evaluation id and no entry in paac_game_step.  Entry points paac_<game>_reset / paac_<game>_step.
PAIRED_GAMES = {"duel": dict(words=12)}
DUEL_STATE_WORDS = PAIRED_GAMES["duel"]["words"]


def duel_reset(seed, env_offset, state_out, stack_out):
    """paac_duel_reset (include/paac_hip.h; spec in paac_amd/duel.py): an even number of rows, two per board."""
    _stateful_reset("paac_duel_reset", DUEL_STATE_WORDS, seed, env_offset, state_out, stack_out)


def duel_step(seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out, ep_reward, ep_len,
              finished=None, stack_out2=None, state_out2=None, truncs_out=None):
    """paac_duel_step: game_step's argument list without the kind; row e also reads actions[(e + N / 2) % N].  truncs_out
    float32[N] (None: not written) as game_step_records'.  The library refuses an odd N, N < 2 and in-place buffers."""
    N, buffers, records = _game_step_ptrs(DUEL_STATE_WORDS, actions, state_in, state_out, state_out2, stack_in, stack_out,
                                          stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished)
    rec = _env_records(N, records, truncs_out)
    _lib.check(_lib.load().paac_duel_step(int(seed), int(env_offset), N, *buffers, ctypes.byref(rec), _stream()), "paac_duel_step")


# The user's game (paac_amd/user_game.py: --emulator user --device_game): DEVICE_GAMES' fields under the kind "user", filled by
# user_game.load() from the specification module once the process holds the library built with the game in it.  A table of its
# own: the games above are the package's, this one is whatever the loaded library was built with.  Entry points
# paac_user_game_reset / paac_user_game_step; paac_game_step and paac_eval_step know the game as _lib.EVAL_USER.
USER_GAMES = {}


def register_user_game(words, step_option=None):
    """-> the USER_GAMES entry of the game compiled into the loaded library (user_game.load checks the numbers against it)."""
    if step_option not in (None, "single_life"):
        raise ValueError("a user game's STEP_OPTION is None or 'single_life', got %r" % (step_option,))
    USER_GAMES["user"] = dict(words=int(words), eval_id=_lib.EVAL_USER, step_option=step_option)
    return USER_GAMES["user"]


def _user_game():
    if "user" not in USER_GAMES:
        raise ValueError("no user game is registered: --emulator user --device_game PATH (paac_amd.user_game.load) does that")
    return USER_GAMES["user"]


def user_game_reset(seed, env_offset, state_out, stack_out):
    """paac_user_game_reset (include/paac_hip.h): game_reset of the user's game."""
    _stateful_reset("paac_user_game_reset", _user_game()["words"], seed, env_offset, state_out, stack_out)


def user_game_step_records(seed, env_offset, actions, state_in, state_out, stack_in, stack_out, rewards_out, masks_out, ep_reward,
                           ep_len, finished=None, stack_out2=None, state_out2=None, truncs_out=None, **option):
    """paac_user_game_step: game_step_records' argument list without the kind -- the records go as one block, truncs_out
    float32[N] (None: not written) among them; `option`: the game's step option by its keyword (False if not given)."""
    game = _user_game()
    name = game["step_option"]
    if set(option) - {name}:
        raise TypeError("user_game_step: unexpected keyword arguments %s" % sorted(set(option) - {name}))
    N, buffers, records = _game_step_ptrs(game["words"], actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2,
                                          rewards_out, masks_out, ep_reward, ep_len, finished)
    rec = _env_records(N, records, truncs_out)
    _lib.check(_lib.load().paac_user_game_step(int(seed), int(env_offset), N, *buffers, ctypes.byref(rec),
                                               int(bool(option.get(name, False))) if name else 0, _stream()),
               "paac_user_game_step")


# one entry serves both: the records always go as a block, with or without the truncation plane
user_game_step = user_game_step_records


def duel_ghost_reset(seed, env_offset, state_out, stack_out, ghost_stack_out):
    """paac_duel_ghost_reset (include/paac_hip.h; spec in paac_amd/duel_pool.py): N boards, the learner's rows and the ghosts'
    observations -- duel_reset on 2N rows, split."""
    N = stack_out.shape[0]
    stacks = _stack_ptrs(N, stack_out=stack_out, ghost_stack_out=ghost_stack_out)
    _lib.check(_lib.load().paac_duel_ghost_reset(int(seed), int(env_offset), N, *_state_ptrs(N, DUEL_STATE_WORDS, state_out=state_out),
                                                 *stacks, _stream()), "paac_duel_ghost_reset")


def duel_ghost_step(seed, env_offset, actions, ghost_probs, sampler_seed, step_base_dev, step_offset, state_in, state_out,
                    stack_in, stack_out, ghost_stack_in, ghost_stack_out, ghost_actions_out, rewards_out, masks_out, ep_reward,
                    ep_len, finished=None, stack_out2=None, state_out2=None, ghost_stack_out2=None, truncs_out=None):
    """paac_duel_ghost_step: one pooled step of N boards -- actions int32 [N] the learner's (bottom) rows', ghost_probs
    float32 [N, 6] the frozen opponent's forward on ghost_stack_in; the ghost's action is sampled on its own Philox stream at
    tick *step_base_dev + step_offset (None: 0) and written to ghost_actions_out int32 [N].  Records and second outputs as
    duel_step's, for the learner's rows; the ghosts get their next observations (and ghost_stack_out2) only.  Shapes are
    checked here; the library refuses N < 1, A != 6, null pointers and in-place buffers before any launch."""
    N, buffers, records = _game_step_ptrs(DUEL_STATE_WORDS, actions, state_in, state_out, state_out2, stack_in, stack_out,
                                          stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished)
    ghost_stacks = _stack_ptrs(N, ("ghost_stack_out2",), ghost_stack_in=ghost_stack_in, ghost_stack_out=ghost_stack_out,
                               ghost_stack_out2=ghost_stack_out2)
    if ghost_probs.dim() != 2 or ghost_probs.shape[0] != N:
        raise ValueError("ghost_probs must be [%d, A], got %s" % (N, tuple(ghost_probs.shape)))
    A = ghost_probs.shape[1]
    env_offset = _env_offset("duel_ghost_step", env_offset, N)
    rec = _env_records(N, records, truncs_out)
    _lib.check(_lib.load().paac_duel_ghost_step(
        int(seed), env_offset, N, buffers[0], _ptr(ghost_probs, torch.float32, N * A, "ghost_probs"), A,
        int(sampler_seed) & 0xFFFFFFFFFFFFFFFF, _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset),
        *buffers[1:], *ghost_stacks, ctypes.byref(rec), _ptr(ghost_actions_out, torch.int32, N, "ghost_actions_out"), _stream()),
        "paac_duel_ghost_step")


def _scored_step_args(fn, words, probs, greedy, eval_seed, noops, step_base_dev, step_offset, env_seed, env_offset, state_in,
                      state_out, stack_in, stack_out, actions_out, score, length, done, alive):
    """paac_eval_step's arguments behind the game id = paac_match_step's, behind the shape checks the two share."""
    if probs.dim() != 2:
        raise ValueError("probs must be [N, A], got %s" % (tuple(probs.shape),))
    N, A = probs.shape
    stacks = _stack_ptrs(N, stack_in=stack_in, stack_out=stack_out)
    states = _state_ptrs(N, words, state_in=state_in, state_out=state_out)
    env_offset = _env_offset(fn, env_offset, N)
    return [_ptr(probs, torch.float32, N * A, "probs"), N, A, 1 if greedy else 0, int(eval_seed) & 0xFFFFFFFFFFFFFFFF, int(noops),
            _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset), int(env_seed) & 0xFFFFFFFFFFFFFFFF,
            env_offset, *states, *stacks, _ptr(actions_out, torch.int32, N, "actions_out"),
            _ptr(score, torch.float32, N, "score"), _ptr(length, torch.int32, N, "length"), _ptr(done, torch.int32, N, "done"),
            _ptr(alive, torch.int32, 1, "alive")]


def eval_step(game, probs, greedy, eval_seed, noops, step_base_dev, step_offset, env_seed, env_offset, state_in, state_out,
              stack_in, stack_out, actions_out, score, length, done, alive):
    """One evaluation step of N environments of `game` ('catch' / 'bricks' / 'rally') on probs [N, A] (include/paac_hip.h:
    paac_eval_step; spec in paac_amd/evaluation.py): the action (no-op, argmax or the evaluation's own Philox stream) into
    actions_out, the game stepped from state_in / stack_in into state_out / stack_out, the first scored episode accounted in
    score / length / done [N] and alive [1].  Shapes are checked here; the library refuses in-place buffers, A outside [2, 32]
    and negative noops with a PaacHipError, before any launch."""
    if game not in EVAL_GAMES and game not in USER_GAMES:
        raise ValueError("eval_step: game %r has no device evaluation (--emulator catch|bricks|rally)" % (game,))
    game_id, words = EVAL_GAMES[game] if game in EVAL_GAMES else (USER_GAMES[game]["eval_id"], USER_GAMES[game]["words"])
    _lib.check(_lib.load().paac_eval_step(game_id, *_scored_step_args("eval_step", words, probs, greedy, eval_seed, noops, step_base_dev,
                                                                      step_offset, env_seed, env_offset, state_in, state_out,
                                                                      stack_in, stack_out, actions_out, score, length, done, alive),
                                          _stream()), "paac_eval_step")


def match_step(probs, greedy, eval_seed, noops, step_base_dev, step_offset, env_seed, env_offset, state_in, state_out,
               stack_in, stack_out, actions_out, score, length, done, alive):
    """One step of a head-to-head match on N / 2 duel boards (include/paac_hip.h: paac_match_step; spec in paac_amd/match.py):
    eval_step's argument list without the game.  probs [N, 6]: rows [0, N / 2) are the bottom players' policy's, rows
    [N / 2, N) the top players'.  Shapes are checked here; the library refuses an odd N, N < 2, A != 6, negative noops and
    in-place buffers with a PaacHipError, before any launch."""
    _lib.check(_lib.load().paac_match_step(*_scored_step_args("match_step", DUEL_STATE_WORDS, probs, greedy, eval_seed, noops,
                                                              step_base_dev, step_offset, env_seed, env_offset, state_in, state_out,
                                                              stack_in, stack_out, actions_out, score, length, done, alive),
                                           _stream()), "paac_match_step")


# Sticky actions (spec and numpy twin: paac_amd/sticky.py; contract: include/paac_hip.h, paac_sticky).
def _sticky_block(N, p, step_base_dev, step_offset, prev_in, prev_out, prev_out2):
    """paac_sticky: the probability, the tick (pointer and offset) and the three int32 [N] planes (prev_out2: None = not
    written).  The library refuses p outside [0, 1), null planes and prev_in == prev_out / prev_out2."""
    planes = _shaped_ptrs((N,), torch.int32, dict(prev_in=prev_in, prev_out=prev_out, prev_out2=prev_out2), ("prev_out2",))
    return _lib.Sticky(float(p), _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset), *planes)


def game_step_sticky(kind, p, step_base_dev, step_offset, prev_in, prev_out, seed, env_offset, actions, state_in, state_out,
                     stack_in, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished=None, stack_out2=None,
                     state_out2=None, truncs_out=None, prev_out2=None, **option):
    """paac_game_step_sticky: game_step_records of `kind` ('catch' / 'bricks' / 'rally', or the registered user game) where
    every environment executes, with probability p, the action it executed on its previous step -- prev_in int32 [N] -- instead
    of actions[e]; the draw is keyed by (seed, env_offset + e, *step_base_dev + step_offset).  prev_out (and prev_out2) get the
    executed action, 0 after a terminal step.  Everything else as game_step_records."""
    game = DEVICE_GAMES[kind] if kind in DEVICE_GAMES else USER_GAMES.get(kind)
    if game is None:
        raise ValueError("game_step_sticky: %r is no device game (catch, bricks, rally or a registered user game)" % (kind,))
    name, words = game["step_option"], game["words"]
    if set(option) - {name}:
        raise TypeError("%s_step: unexpected keyword arguments %s" % (kind, sorted(set(option) - {name})))
    N, buffers, records = _game_step_ptrs(words, actions, state_in, state_out, state_out2, stack_in, stack_out, stack_out2,
                                          rewards_out, masks_out, ep_reward, ep_len, finished)
    rec = _env_records(N, records, truncs_out)
    sticky = _sticky_block(N, p, step_base_dev, step_offset, prev_in, prev_out, prev_out2)
    _lib.check(_lib.load().paac_game_step_sticky(game["eval_id"], int(seed), _env_offset("game_step_sticky", env_offset, N), N,
                                                 *buffers, ctypes.byref(rec), int(bool(option.get(name, False))) if name else 0,
                                                 ctypes.byref(sticky), _stream()), "paac_game_step_sticky")


def duel_step_sticky(p, step_base_dev, step_offset, prev_in, prev_out, seed, env_offset, actions, state_in, state_out, stack_in,
                     stack_out, rewards_out, masks_out, ep_reward, ep_len, finished=None, stack_out2=None, state_out2=None,
                     truncs_out=None, prev_out2=None):
    """paac_duel_step_sticky: duel_step with sticky actions, keyed per ROW (env_offset + e): the two players of a board stick
    independently, and both rows of a board work out the same pair of executed actions."""
    N, buffers, records = _game_step_ptrs(DUEL_STATE_WORDS, actions, state_in, state_out, state_out2, stack_in, stack_out,
                                          stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished)
    rec = _env_records(N, records, truncs_out)
    sticky = _sticky_block(N, p, step_base_dev, step_offset, prev_in, prev_out, prev_out2)
    _lib.check(_lib.load().paac_duel_step_sticky(int(seed), _env_offset("duel_step_sticky", env_offset, N), N, *buffers,
                                                 ctypes.byref(rec), ctypes.byref(sticky), _stream()), "paac_duel_step_sticky")


def eval_step_sticky(game, p, prev_in, prev_out, probs, greedy, eval_seed, noops, step_base_dev, step_offset, env_seed, env_offset,
                     state_in, state_out, stack_in, stack_out, actions_out, score, length, done, alive):
    """paac_eval_step_sticky: eval_step where the game executes, with probability p, the previous step's executed action
    (prev_in int32 [N] -> prev_out) instead of the chosen one; actions_out keeps the chosen action.  The draw's key is
    eval_seed, its stream the evaluation's own (sticky.EVAL_STREAM_STICKY)."""
    if game not in EVAL_GAMES and game not in USER_GAMES:
        raise ValueError("eval_step_sticky: game %r has no device evaluation (--emulator catch|bricks|rally)" % (game,))
    game_id, words = EVAL_GAMES[game] if game in EVAL_GAMES else (USER_GAMES[game]["eval_id"], USER_GAMES[game]["words"])
    args = _scored_step_args("eval_step_sticky", words, probs, greedy, eval_seed, noops, step_base_dev, step_offset, env_seed,
                             env_offset, state_in, state_out, stack_in, stack_out, actions_out, score, length, done, alive)
    planes = _shaped_ptrs((probs.shape[0],), torch.int32, dict(prev_in=prev_in, prev_out=prev_out), ())
    _lib.check(_lib.load().paac_eval_step_sticky(game_id, *args, float(p), *planes, _stream()), "paac_eval_step_sticky")


FUSED_SAMPLE_MAX_DRAWS = 2304
ACT_STEP_MAX_DRAWS = 1024
ACT_STEP_MAX_ENVS = 64
ACT_PIPE_MAX_ACTIONS = 31        # paac_act_step_pipe: two regions of head partials in the acting fc slab buffer
ACT_STEP_MAX_ENVS_LARGE = 256    # paac_act_step_mt's four-launch form (large shards)
KEEP_FORWARD_MAX_ROWS = 256      # paac_keep_next_forward: acting forwards of up to this many rows (csrc/fc_heads.h)


def walk_scratch(N, A, device):
    """Zero-initialised scratch that lets the large shards' sampler spread its walk over several workgroups
    (include/paac_hip.h: paac_sample_mt_synth_step); lend the same tensor to every call of one (N, A)."""
    return torch.zeros(int(_lib.load().paac_walk_scratch_bytes(int(N), int(A))), dtype=torch.uint8, device=device)


def sample_mt_synth_step(probs, mt_state, actions, seed, env_offset, terminal_threshold, step_base_dev, step_offset,
                         stack_in, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished=None, stack_out2=None,
                         walk_scratch=None, raw_scratch=None):
    N, A = probs.shape
    if N * (A - 1) > FUSED_SAMPLE_MAX_DRAWS:
        raise ValueError("fused sampler+env step supports N*(A-1) <= %d" % FUSED_SAMPLE_MAX_DRAWS)
    step = _step_ptrs(N, stack_out, rewards_out, masks_out, ep_reward, ep_len, finished, stack_out2, stack_in=stack_in)
    _lib.check(_lib.load().paac_sample_mt_synth_step(
        _ptr(probs, torch.float32, N * A, "probs"), A, _ptr(mt_state, torch.int32, 625, "mt_state"),
        _ptr(actions, torch.int32, N, "actions"), int(seed), int(env_offset), N, int(terminal_threshold),
        _ptr(step_base_dev, torch.int64, 1, "step_base", True), int(step_offset),
        _ptr(stack_in, torch.uint8, N * 28224, "stack_in"), *step,
        *_lent(walk_scratch), _ptr(raw_scratch, torch.uint8, N * 2 * RAW_H * RAW_W, "raw_scratch", True), _stream()),
        "paac_sample_mt_synth_step")


def pin_host_array(t):
    """Page-lock the memory of a CPU tensor in place (hipHostRegister through torch's runtime handle) so that copies to
    the device are asynchronous DMAs.  Returns True when the registration succeeded; a failure only costs speed."""
    try:
        rc = torch.cuda.cudart().cudaHostRegister(t.data_ptr(), t.numel() * t.element_size(), 0)
        return int(rc) == 0
    except Exception:
        return False


def unpin_host_array(t):
    """Undo pin_host_array once nothing on the device reads the memory any more.  A registration left behind outlives the
    memory it covers: a later allocation at an overlapping address (the multiprocessing heap hands freed shared blocks
    out again) is then resolved to the stale, smaller registration and copies from it fail with an invalid argument."""
    torch.cuda.cudart().cudaHostUnregister(t.data_ptr())


class Graph(object):
    """hipGraph captured from the launches issued on torch's current stream between begin() and end()."""

    def __init__(self):
        self.lib = _lib.load()
        self.handle = None

    def begin(self):
        # A finalizer that frees device memory (a collected Context or tensor) in the middle of a capture
        # invalidates it: collect now and keep the collector off until end().
        gc.collect()
        self._gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            _lib.check(self.lib.paac_graph_begin(_stream()), "paac_graph_begin")
        except Exception:
            self._restore_gc()
            raise

    def _restore_gc(self):
        if getattr(self, "_gc_was_enabled", False):
            gc.enable()
        self._gc_was_enabled = False

    def end(self):
        h = ctypes.c_void_p()
        try:
            _lib.check(self.lib.paac_graph_end(_stream(), ctypes.byref(h)), "paac_graph_end")
        finally:
            self._restore_gc()
        self.handle = h

    def abort(self):
        """Leave capture mode after a failed capture, dropping whatever was recorded."""
        h = ctypes.c_void_p()
        try:
            if self.lib.paac_graph_end(_stream(), ctypes.byref(h)) == 0 and h:
                self.lib.paac_graph_destroy(h)
        finally:
            self._restore_gc()

    def launch(self):
        _lib.check(self.lib.paac_graph_launch(self.handle, _stream()), "paac_graph_launch")

    def close(self):
        if self.handle:
            self.lib.paac_graph_destroy(self.handle)
            self.handle = None
