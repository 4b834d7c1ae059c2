"""Base learner (mirrors reference actor_learner.py:11-127).

Holds what the reference's ActorLearner holds -- hyper-parameters, the environments, the network, the
optimizer state (RMSProp, or Adam with --optimizer adam), savers, lr schedule, reward clipping, checkpoint cadence --
with the TensorFlow optimizer graph (compute_gradients / clip_by_global_norm / apply_gradients, :31-70) replaced by
paac_loss_backward + paac_clip_rmsprop (paac_clip_adam) on a flat parameter buffer.
"""
import logging
import math
import os

import numpy as np
import torch

from . import _lib, hip_ops, parallel, window_stats
from .networks import Placeholder
from .session import Saver, Session, checkpoint_key, tensor_of_key

CHECKPOINT_INTERVAL = 1000000      # actor_learner.py:8


class ActorLearner(object):

    def __init__(self, network_creator, environment_creator, args):
        self.global_step = 0
        self.max_local_steps = args.max_local_steps
        self.num_actions = args.num_actions
        self.initial_lr = args.initial_lr
        self.lr_annealing_steps = args.lr_annealing_steps
        self.emulator_counts = args.emulator_counts
        self.device = args.device
        self.debugging_folder = args.debugging_folder
        self.network_checkpoint_folder = os.path.join(self.debugging_folder, 'checkpoints/')
        self.optimizer_checkpoint_folder = os.path.join(self.debugging_folder, 'optimizer_checkpoints/')
        self.last_saving_step = 0

        # RMSPropOptimizer(lr, decay=alpha, epsilon=e): momentum 0.0, rms slot init 1.0 (actor_learner.py:31-34); or
        # --optimizer adam: AdamOptimizer(lr, beta1, beta2, epsilon=e), the alternative train.py's --e help names
        # (args.json files and Namespaces from before the flag lack the fields: RMSProp)
        self.learning_rate = Placeholder('learning_rate')
        self.optimizer = getattr(args, "optimizer", "rmsprop")
        if self.optimizer not in ("rmsprop", "adam"):
            raise ValueError("optimizer %r: expected 'rmsprop' or 'adam'" % (self.optimizer,))
        self.alpha = args.alpha
        self.e = args.e
        self.momentum = 0.0
        self.beta1 = float(getattr(args, "beta1", 0.9))
        self.beta2 = float(getattr(args, "beta2", 0.999))
        if self.optimizer == "adam" and not (0.0 <= self.beta1 < 1.0 and 0.0 <= self.beta2 < 1.0 and self.e > 0.0):
            raise ValueError("Adam needs 0 <= beta1, beta2 < 1 and e > 0 (beta1=%r, beta2=%r, e=%r)"
                             % (self.beta1, self.beta2, self.e))
        # --gae_lambda: 1.0 (and Namespaces / args.json files from before the flag) = the reference's n-step return through
        # the n-step kernels; anything else in [0, 1] = GAE(lambda) (hip_ops.uses_gae is the one routing rule)
        self.gae_lambda = float(getattr(args, "gae_lambda", 1.0))
        if not 0.0 <= self.gae_lambda <= 1.0:           # (NaN fails both comparisons)
            raise ValueError("gae_lambda %r: expected a value in [0, 1]" % (self.gae_lambda,))
        # --ppo_epochs K / --ppo_clip EPS (include/paac_hip.h has the contract): K = 1 (and Namespaces / args.json files from
        # before the flags) = one update per rollout through today's calls; EPS is read only when K > 1
        self.ppo_epochs = getattr(args, "ppo_epochs", 1)
        if isinstance(self.ppo_epochs, bool) or self.ppo_epochs != int(self.ppo_epochs) or \
                not 1 <= int(self.ppo_epochs) <= _lib.PPO_EPOCHS_MAX:
            raise ValueError("ppo_epochs %r: expected an integer in [1, %d] (a captured cycle grows by about ten launches per "
                             "epoch)" % (self.ppo_epochs, _lib.PPO_EPOCHS_MAX))
        self.ppo_epochs = int(self.ppo_epochs)
        self.ppo_clip = float(getattr(args, "ppo_clip", 0.2))
        if not 0.0 < self.ppo_clip < 1.0:               # (NaN fails both comparisons)
            raise ValueError("ppo_clip %r: expected a value in (0, 1)" % (self.ppo_clip,))
        # --adv_norm / --ppo_vclip EPSV (include/paac_hip.h has the contracts): Namespaces / args.json files without the fields
        # mean off.  adv_norm: the actor term reads the rollout's advantages normalised by their own mean and std (every
        # epoch); EPSV > 0: epochs 2..K use the value-clipped critic term, read only when K > 1
        self.adv_norm = getattr(args, "adv_norm", False)
        if not isinstance(self.adv_norm, (bool, np.bool_)):
            raise ValueError("adv_norm %r: expected True or False" % (self.adv_norm,))
        self.adv_norm = bool(self.adv_norm)
        # --bootstrap_truncated (include/paac_hip.h: paac_returns.truncs has the contract): Namespaces / args.json files without
        # the field mean off.  On: the loops carry a truncation plane beside the masks (paac.py) where the game has a step cap
        self.bootstrap_truncated = getattr(args, "bootstrap_truncated", False)
        if not isinstance(self.bootstrap_truncated, (bool, np.bool_)):
            raise ValueError("bootstrap_truncated %r: expected True or False" % (self.bootstrap_truncated,))
        self.bootstrap_truncated = bool(self.bootstrap_truncated)
        # --window_stats (paac_amd/window_stats.py): Namespaces / args.json files without the field mean off
        self.window_stats = window_stats.check_flags(args)
        self.ppo_vclip = float(getattr(args, "ppo_vclip", 0.0))
        if not (0.0 <= self.ppo_vclip and math.isfinite(self.ppo_vclip)):          # (NaN fails the comparison)
            raise ValueError("ppo_vclip %r: expected a finite value >= 0 (0 = off)" % (self.ppo_vclip,))
        self.vclip_on = self.ppo_epochs > 1 and self.ppo_vclip > 0.0
        # --ppo_minibatches M (include/paac_hip.h has the contract): Namespaces / args.json files without the field, and M = 1,
        # mean full-batch epochs through today's calls; M > 1 is read only when K > 1 and turns the cycle into K epochs of M
        # shuffled minibatches (K * M optimizer steps, none of them full-batch)
        M = getattr(args, "ppo_minibatches", 1)
        if isinstance(M, (bool, np.bool_)) or not isinstance(M, (int, float, np.integer, np.floating)) or M != M or \
                M != int(M) or not 1 <= int(M) <= _lib.PPO_MINIBATCHES_MAX:
            raise ValueError("ppo_minibatches %r: expected an integer in [1, %d]" % (M, _lib.PPO_MINIBATCHES_MAX))
        self.ppo_minibatches = int(M)
        self.minibatch_on = self.ppo_epochs > 1 and self.ppo_minibatches > 1
        if self.minibatch_on:
            rows = args.emulator_counts * args.max_local_steps
            if rows % self.ppo_minibatches:
                raise ValueError("ppo_minibatches %d does not divide the rollout's %d rows (emulator_counts x max_local_steps)"
                                 % (self.ppo_minibatches, rows))
            if self.ppo_epochs * self.ppo_minibatches > _lib.PPO_STEPS_MAX:
                raise ValueError("ppo_minibatches %d x ppo_epochs %d: more than %d optimizer steps per rollout (a captured cycle "
                                 "grows by about ten launches per step)" % (self.ppo_minibatches, self.ppo_epochs,
                                                                            _lib.PPO_STEPS_MAX))
            if rows > _lib.MINIBATCH_MAX_ROWS:
                raise ValueError("ppo_minibatches above 1 needs a rollout of at most %d rows (the shuffle is one workgroup's LDS "
                                 "sort), got %d" % (_lib.MINIBATCH_MAX_ROWS, rows))
        # optimizer steps of one cycle = rows of ppo_loss / ppo_stats
        self.ppo_steps = self.ppo_epochs * (self.ppo_minibatches if self.minibatch_on else 1)
        # --ppo_target_kl D (include/paac_hip.h has the contract): Namespaces / args.json files without the field, and 0, mean
        # off; D > 0 is read only when K > 1: a gated step (one whose backward writes a ppo_stats row) whose approx_kl exceeds
        # float32(1.5 * D) is skipped on the device, with every step after it in the cycle
        D = getattr(args, "ppo_target_kl", 0.0)
        if isinstance(D, (bool, np.bool_)) or not isinstance(D, (int, float, np.integer, np.floating)) or \
                not (0.0 <= float(D) and math.isfinite(float(D))):          # (NaN fails the comparison)
            raise ValueError("ppo_target_kl %r: expected a finite number >= 0 (0 = off)" % (D,))
        self.ppo_target_kl = float(D)
        self.target_kl_on = self.ppo_epochs > 1 and self.ppo_target_kl > 0.0
        self.kl_thr = float(np.float32(1.5 * self.ppo_target_kl))
        self.first_gated_step = 0 if self.minibatch_on else 1
        self.clip_norm = args.clip_norm
        self.clip_norm_type = args.clip_norm_type
        if self.clip_norm_type == 'ignore':
            self.clip_mode = _lib.CLIP_IGNORE
        elif self.clip_norm_type == 'global':
            self.clip_mode = _lib.CLIP_GLOBAL
        elif self.clip_norm_type == 'local':
            # tf.clip_by_norm of every variable's gradient on its own (weights and biases separately).  Upstream's branch
            # cannot run: actor_learner.py:62-63 hands each (grad, var) tuple to tf.clip_by_norm instead of the gradient;
            # this is the branch's evident intent (its comment, the help text, the global_norm line after it)
            self.clip_mode = _lib.CLIP_LOCAL
        else:
            raise Exception('Norm type not recognized')

        self.environment_creator = environment_creator
        self.emulators = np.asarray([environment_creator.create_environment(i)
                                     for i in range(self.emulator_counts)])
        self.max_global_steps = args.max_global_steps
        self.gamma = args.gamma
        self.game = args.game
        self.network = network_creator()
        self.entropy_beta = float(self.network.entropy_regularisation_strength)

        dev = self.network.torch_device
        torch.cuda.set_device(dev)
        self.torch_device = dev
        n = self.network.layout["total"]
        # the gradient store: what the exchange sends.  --ppo_target_kl under data parallelism: 4 floats behind the gradient,
        # element n carrying the step's approx_kl through the step's one all-reduce; self.grad stays the n-float view every
        # kernel sees
        self.kl_in_store = self.target_kl_on and parallel.collectives_active()
        self.grad_store = torch.zeros(n + (4 if self.kl_in_store else 0), dtype=torch.float32, device=dev)
        self.grad = self.grad_store[:n]
        if self.optimizer == "adam":
            # slots m, v (zeros) and the fp32 bias-correction powers {beta1_power, beta2_power}, advanced on the device
            self.adam_m = torch.zeros(n, dtype=torch.float32, device=dev)
            self.adam_v = torch.zeros(n, dtype=torch.float32, device=dev)
            self.beta_powers = torch.tensor([self.beta1, self.beta2], dtype=torch.float32, device=dev)
            self.optimizer_state = [("m", self.adam_m), ("v", self.adam_v), ("beta_powers", self.beta_powers)]
        else:
            self.rms = torch.ones(n, dtype=torch.float32, device=dev)     # .meta: OptimizerVariables init 1.0
            self.mom = torch.zeros(n, dtype=torch.float32, device=dev)    # .meta: OptimizerVariables_1 zeros
            self.optimizer_state = [("rms", self.rms), ("mom", self.mom)]
        # the ONE list of what an optimizer step reads and writes besides the gradient: replica checks, the data-parallel
        # broadcast, the graph-replay snapshot and the checkpoints' consistency all go through it
        self.update_state = [("params", self.network.params)] + self.optimizer_state
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.gnorm_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_dev = torch.zeros(4, dtype=torch.float32, device=dev)
        # --ppo_epochs: per-cycle scratch, nothing of it is checkpointed.  p_old [T*N]; row k of ppo_loss / ppo_stats = the
        # loss scalars / {clip_fraction, approx_kl} of epoch k + 1 (row 0 stays zero: epoch 1 reports through loss_dev, and its
        # ratio is identically 1)
        self.p_old = self.ppo_loss = self.ppo_stats = None
        if self.ppo_epochs > 1:
            self.p_old = torch.zeros(self.emulator_counts * self.max_local_steps, dtype=torch.float32, device=dev)
            self.ppo_loss = torch.zeros((self.ppo_steps, 4), dtype=torch.float32, device=dev)
            self.ppo_stats = torch.zeros((self.ppo_steps, 3 if self.vclip_on else 2), dtype=torch.float32, device=dev)
        # --ppo_target_kl: per-cycle scratch like the above.  kl_stop = the cycle's sticky stop flag; row s of ppo_applied /
        # ppo_kl_checked = was gated step s applied / the value its gate compared (ungated step 0 of an M = 1 cycle: 1 / 0)
        self.kl_stop = self.ppo_applied = self.ppo_kl_checked = None
        if self.target_kl_on:
            self.kl_stop = torch.zeros(1, dtype=torch.int32, device=dev)
            self.ppo_applied = torch.ones(self.ppo_steps, dtype=torch.int32, device=dev)
            self.ppo_kl_checked = torch.zeros(self.ppo_steps, dtype=torch.float32, device=dev)
        # --adv_norm: adv_n [T*N] is what the actor term reads, adv_stats = {mean, std} of the last rollout (fp64);
        # --ppo_vclip: v_old [T*N], epoch 1's values.  Per-cycle scratch like p_old
        self.adv_n = self.adv_stats = self.v_old = None
        if self.adv_norm:
            self.adv_n = torch.zeros(self.emulator_counts * self.max_local_steps, dtype=torch.float32, device=dev)
            self.adv_stats = torch.zeros(2, dtype=torch.float64, device=dev)
        if self.vclip_on:
            self.v_old = torch.zeros(self.emulator_counts * self.max_local_steps, dtype=torch.float32, device=dev)
        # --ppo_minibatches: the K shuffles of the cycle and the staging block one gather per epoch fills (allocated once: a
        # replayed graph sees fixed addresses); row s = e * M + j of ppo_loss / ppo_stats = minibatch j + 1 of epoch e + 1.
        # v_rec = the values the record pass reads out of the training-side heads: the rollout rows' (v_old is its head under
        # --ppo_vclip) and, in the device loop, the bootstrap rows' behind them
        self.mb = None
        if self.minibatch_on:
            rows = self.emulator_counts * self.max_local_steps
            f32 = lambda: torch.zeros(rows, dtype=torch.float32, device=dev)
            self.v_rec = torch.zeros(rows + self.emulator_counts, dtype=torch.float32, device=dev)
            if self.vclip_on:
                self.v_old = self.v_rec[:rows]
            self.mb = dict(perms=torch.zeros((self.ppo_epochs, rows), dtype=torch.int32, device=dev),
                           states=torch.zeros((rows, 84, 84, 4), dtype=torch.uint8, device=dev),
                           actions=torch.zeros(rows, dtype=torch.int32, device=dev), y=f32(), adv=f32(), p_old=f32(),
                           v_old=f32() if self.vclip_on else None)
        self.train_step = Placeholder('train_step')

        self.ctx = hip_ops.Context(self.network.arch_id, self.num_actions,
                                   max_batch=self.emulator_counts * (self.max_local_steps + 1),   # + bootstrap rows
                                   device_index=dev.index or 0)
        self.session = Session(self.network, self.ctx, learner=self)
        # the learner owns every write to the parameters: the optimizer step re-packs the conv weights for the fused conv
        # launch itself; host-side writes (set_parameters, restore, broadcast) go through weights_changed
        self.ctx.set_managed_weights(True)
        self.network.weights_changed = lambda: self.ctx.pack_weights(self.network.params)
        self.ctx.pack_weights(self.network.params)

        self.network_saver = self.network.make_saver()
        self.optimizer_saver = Saver(self._get_optimizer_arrays, self._set_optimizer_arrays, max_to_keep=1)
        fmt = getattr(args, "checkpoint_format", None)
        if fmt:
            self.network_saver.fmt = self.optimizer_saver.fmt = fmt
        if self.network_saver.fmt == "tf":
            # the reference's network saver is tf.train.Saver() over ALL variables, optimizer slots included
            # (actor_learner.py:79): a bundle its restore accepts holds them too
            variables = self.network_saver.get_arrays
            self.network_saver.get_arrays = lambda: dict(variables(), **self._get_optimizer_arrays())

    # -- optimizer slots under the reference's names ('<var>/OptimizerVariables', '<var>/OptimizerVariables_1') ----
    # Both optimizers are named 'OptimizerVariables', so TF gives their two slots the same keys: RMSProp ms / momentum,
    # Adam m / v.  Adam's beta1_power / beta2_power are top-level variables ('beta1_power', 'beta2_power').  Upstream's
    # optimizer saver keeps only variables whose name contains 'OptimizerVariables' and would drop them -- a resumed run
    # would restart bias correction from step 1 with trained moments.  This build writes them to the optimizer checkpoint
    # (and, with --checkpoint_format tf, to the all-variables network bundle), deliberately.
    ADAM_POWER_KEYS = ("beta1_power", "beta2_power")

    def _slot_tensors(self):
        if self.optimizer == "adam":
            return (("OptimizerVariables", self.adam_m), ("OptimizerVariables_1", self.adam_v))
        return (("OptimizerVariables", self.rms), ("OptimizerVariables_1", self.mom))

    def _get_optimizer_arrays(self):
        scope = self.network.name
        out = {}
        for slot, flat in self._slot_tensors():
            for k, v in self.network.get_parameters(flat).items():
                out[checkpoint_key(scope, k, slot)] = v
        if self.optimizer == "adam":
            powers = self.beta_powers.cpu().numpy()
            for i, key in enumerate(self.ADAM_POWER_KEYS):
                out[key] = np.float32(powers[i]).reshape(())
        return out

    def _set_optimizer_arrays(self, d):
        lay = self.network.layout
        adam = self.optimizer == "adam"
        if adam and not all(k in d for k in self.ADAM_POWER_KEYS):
            raise KeyError("optimizer checkpoint has no beta1_power / beta2_power: it was written by an RMSProp run "
                           "(--optimizer rmsprop), and this learner runs Adam (--optimizer adam) -- its slots would be "
                           "read as Adam's moments")
        host = {"OptimizerVariables": (np.zeros if adam else np.ones)(lay["total"], dtype=np.float32),
                "OptimizerVariables_1": np.zeros(lay["total"], dtype=np.float32)}
        where = {t["name"]: t for t in lay["tensors"]}
        seen = set()
        for key, value in d.items():
            name, slot = tensor_of_key(key)
            if slot is None:         # a variable (the reference's all-variables bundle) or Adam's powers: not a slot
                continue
            t = where[name]
            host[slot][t["offset"]:t["offset"] + t["size"]] = np.asarray(value, dtype=np.float32).reshape(-1)
            seen.add((name, slot))
        if len(seen) != 2 * len(where):
            raise KeyError("optimizer checkpoint holds %d of %d slot tensors" % (len(seen), 2 * len(where)))
        for slot, flat in self._slot_tensors():
            flat.copy_(torch.from_numpy(host[slot]))
        if adam:
            powers = [np.float32(np.asarray(d[k], dtype=np.float32).reshape(())) for k in self.ADAM_POWER_KEYS]
            self.beta_powers.copy_(torch.from_numpy(np.array(powers, dtype=np.float32)))

    # -- the optimizer step on self.grad (already all-reduced): one place for the loops and the feed-dict path ----
    def is_gated_step(self, step):
        """--ppo_target_kl: is optimizer step `step` of a cycle one the gate decides on (its backward wrote ppo_stats[step])?"""
        return self.target_kl_on and step is not None and self.first_gated_step <= step < self.ppo_steps

    def _kl_into_store(self, s):
        """--ppo_target_kl, data parallel: gated step s's approx_kl rides behind its gradient through the step's all-reduce (one
        4-byte device copy right after the backward that wrote it, captured like the v_old copy)."""
        if self.kl_in_store and self.is_gated_step(s):
            self.grad_store[self.grad.numel():self.grad.numel() + 1].copy_(self.ppo_stats[s, 1:2])

    def apply_gradients(self, step=None):
        """The optimizer step on self.grad.  step: its index in the cycle; a gated step (--ppo_target_kl) goes through the gated
        entry, the first gated step of the cycle clearing the sticky stop flag.  None: ungated, whatever the flags say."""
        adam = self.optimizer == "adam"
        rule = ((self.adam_m, self.adam_v, self.beta_powers, self.lr_dev, self.beta1, self.beta2) if adam else
                (self.rms, self.mom, self.lr_dev, self.alpha, self.momentum))
        gate = {}
        if self.is_gated_step(step):
            n = self.grad.numel()
            gate = dict(kl=self.grad_store[n:] if self.kl_in_store else self.ppo_stats[step, 1:2],
                        kl_scale=self._grad_scale() if self.kl_in_store else 1.0, thr=self.kl_thr,
                        first=step == self.first_gated_step, stop=self.kl_stop, applied=self.ppo_applied[step:step + 1],
                        checked=self.ppo_kl_checked[step:step + 1])
        entry = getattr(self.ctx, ("clip_adam" if adam else "clip_rmsprop") + ("_gated" if gate else ""))
        entry(self.network.params, self.grad, *rule, self.e, self.clip_norm, self.clip_mode, self._grad_scale(), self.gnorm_dev,
              **gate)

    def _surrogate_backward(self, slot, states, actions, y, adv, p_old, v_old, phase):
        """The clipped-surrogate backward behind a finished training forward (trunk) into self.grad, loss and statistics into
        row `slot` of ppo_loss / ppo_stats; with --ppo_vclip the critic term is clipped around the frozen v_old."""
        params = self.network.params
        if self.vclip_on:
            self.ctx.loss_backward_ppo_vclip(params, states, actions, y, adv, p_old, v_old, self.ppo_clip, self.ppo_vclip,
                                             self.entropy_beta, self.grad, self.ppo_loss[slot], self.ppo_stats[slot],
                                             forward_done=True, phase=phase)
        else:
            self.ctx.loss_backward_ppo(params, states, actions, y, adv, p_old, self.ppo_clip, self.entropy_beta, self.grad,
                                       self.ppo_loss[slot], self.ppo_stats[slot], forward_done=True, phase=phase)
        self._kl_into_store(slot)

    def ppo_epoch_backward(self, k, states, actions, y, adv, phase):
        """Epoch k + 1 (k = 1 .. ppo_epochs - 1) up to its gradient: training forward (trunk) over the rollout rows on the
        current weights, then the clipped-surrogate backward on the frozen y / adv / p_old (adv: what the actor term reads,
        adv_n under --adv_norm; with --ppo_vclip the critic term is clipped around the frozen v_old)."""
        self.ctx.train_forward_trunk(self.network.params, states)
        self._surrogate_backward(k, states, actions, y, adv, self.p_old, self.v_old if self.vclip_on else None, phase)

    def minibatch_record(self, actions, value_rows):
        """The record pass of an M > 1 cycle on the pending training forward (pre-update weights): p_old, and the values of
        the training set's first value_rows rows into v_rec (v_old; rows past T*N are the appended bootstrap rows')."""
        self.ctx.record_policy(self.network.params, actions, actions.numel(), self.p_old, self.v_rec, value_rows)

    def minibatch_perms(self, seed, step_base_dev, step_offset=0):
        """The cycle's K shuffles in one launch."""
        hip_ops.minibatch_perms(self.mb["perms"].shape[1], seed, step_base_dev, step_offset, self.mb["perms"])

    def minibatch_step_backward(self, s, states, actions, y, adv, phase):
        """Optimizer step s = e * M + j of an M > 1 cycle up to its gradient: at j == 0 epoch e's gather of the frozen rollout
        (states, actions, y, adv = what the actor term reads, p_old, v_old) into the staging block, then the training forward
        (trunk) over minibatch j's rows of it and the clipped-surrogate backward with batch = T*N / M."""
        mb, M = self.mb, self.ppo_minibatches
        e, j = divmod(s, M)
        if j == 0:
            hip_ops.gather_minibatch(mb["perms"][e], states, mb["states"], actions, mb["actions"], y, mb["y"], adv, mb["adv"],
                                     self.p_old, mb["p_old"], self.v_old if self.vclip_on else None, mb["v_old"])
        b = mb["perms"].shape[1] // M
        r = slice(j * b, (j + 1) * b)
        self.ctx.train_forward_trunk(self.network.params, mb["states"][r])
        self._surrogate_backward(s, mb["states"][r], mb["actions"][r], mb["y"][r], mb["adv"][r], mb["p_old"][r],
                                 mb["v_old"][r] if self.vclip_on else None, phase)

    # -- one optimizer step from a reference-style feed dict (Session.run([train_step, ...], feed)) ----
    def _train_step_from_feed(self, feed_dict):
        net = self.network
        dev = self.torch_device
        states = torch.from_numpy(np.ascontiguousarray(np.asarray(feed_dict[net.input_ph]).astype(np.uint8))).to(dev)
        onehot = np.asarray(feed_dict[net.selected_action_ph])
        actions = torch.from_numpy(np.argmax(onehot, axis=1).astype(np.int32)).to(dev)
        y = torch.from_numpy(np.asarray(feed_dict[net.critic_target_ph]).astype(np.float32)).to(dev)
        adv = torch.from_numpy(np.asarray(feed_dict[net.adv_actor_ph]).astype(np.float32)).to(dev)
        self.lr_dev.fill_(float(np.float32(feed_dict[self.learning_rate])))
        self.ctx.loss_backward(net.params, states, actions, y, adv, self.entropy_beta, self.grad, self.loss_dev)
        self._allreduce_grad()
        self.apply_gradients()

    # -- data parallel: one sum all-reduce of the flat gradient per update (paac_amd/parallel.py) ------
    @staticmethod
    def _world():
        return parallel.world_size()

    def _grad_scale(self):
        return parallel.grad_scale()

    def _allreduce_grad(self):
        parallel.allreduce_sum_(self.grad_store)

    # -- reference methods (actor_learner.py:89-127): same names and behaviour ------------------------------
    def save_vars(self, force=False):
        """Network + optimizer checkpoints once CHECKPOINT_INTERVAL global steps have passed since the last one (or
        when forced).  Data parallel: the replicas are identical, rank 0 writes, every rank keeps the same cadence."""
        due = force or (self.global_step - self.last_saving_step) >= CHECKPOINT_INTERVAL
        if not due:
            return
        self.last_saving_step = self.global_step
        self._sync_device()                    # nothing in flight: weights and optimizer state belong to the same update
        if parallel.rank() == 0:
            for saver, folder in ((self.network_saver, self.network_checkpoint_folder),
                                  (self.optimizer_saver, self.optimizer_checkpoint_folder)):
                saver.save(self.session, folder, global_step=self.last_saving_step)
        parallel.barrier()

    def _sync_device(self):
        torch.cuda.synchronize(self.torch_device)

    def rescale_reward(self, reward):
        """Immediate reward clipped to [-1, 1] (actor_learner.py:95-101)."""
        return min(1.0, max(-1.0, reward))

    def init_network(self):
        """Restore the latest network / optimizer checkpoints if present, else initialise (actor_learner.py:103-117,
        networks.py:122-135); returns the global step to resume from.  Data parallel: every rank restores (or
        initialises), then rank 0's weights and optimizer slots are broadcast so the replicas start identical."""
        for folder in (self.network_checkpoint_folder, self.optimizer_checkpoint_folder):
            os.makedirs(folder, exist_ok=True)
        resumed_step = self.network.init(self.network_checkpoint_folder, self.network_saver, self.session)
        optimizer_checkpoint = Saver.latest_checkpoint(self.optimizer_checkpoint_folder)
        if optimizer_checkpoint is not None:
            logging.info('Restoring optimizer variables from previous run')
            self.optimizer_saver.restore(self.session, optimizer_checkpoint)
            # save_vars writes the network first and the optimizer second, and a torn newest file is skipped on resume:
            # the two can come from different updates (upstream has the same window, silently)
            optimizer_step = Saver.step_of(optimizer_checkpoint)
            if optimizer_step is not None and optimizer_step != int(resumed_step):
                logging.warning('Optimizer checkpoint is from step %d, network checkpoint from step %d: resuming with '
                                'weights and optimizer statistics of different updates', optimizer_step, int(resumed_step))
        if parallel.world_size() > 1:
            step = torch.tensor([int(resumed_step)], dtype=torch.int64, device=self.torch_device)
            for t in [t for _, t in self.update_state] + [step]:
                parallel.broadcast_(t, src=0)
            self.network.weights_changed()
            resumed_step = int(step.item())
        return resumed_step          # like upstream, last_saving_step stays 0: a resumed run checkpoints on its first cycle

    def get_lr(self):
        """Linear anneal to zero over lr_annealing_steps (actor_learner.py:119-123)."""
        if self.global_step > self.lr_annealing_steps:
            return 0.0
        return self.initial_lr - (self.global_step * self.initial_lr / self.lr_annealing_steps)

    def cleanup(self):
        self.save_vars(True)
        self.session.close()
