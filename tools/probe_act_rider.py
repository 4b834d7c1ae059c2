"""Diagnostic (stamped build only): the sampler workgroup INSIDE a ridden acting fc launch (paac_act_step_pipe), beside the fc
workgroups it shares the CUs with -- tools/probe_sampler.py stamps it with a CU to itself.  Wall-clock stamps (10 ns ticks) of the
last ridden launch of each run of T pipelined steps, and the launches' durations from the events on their dispatches.
PAAC_HIP_LIB=.../libpaac_hip_stamps.so [PAAC_ACT_TOWER_RIDER=0|1|2] [PROBE_KEEP=1] python tools/probe_act_rider.py
profiles/r10_rider_stamps.txt is this at 32 x 4 on the parent and on the build."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from paac_amd import hip_ops, _lib
from paac_amd.synthetic import terminal_threshold
lib = _lib.load()
lib.paac_debug_set_misc_stamps.argtypes = [ctypes.c_void_p]
N, A, T = int(os.environ.get("PROBE_N", "32")), int(os.environ.get("PROBE_A", "4")), int(os.environ.get("PROBE_T", "5"))
dev = torch.device("cuda", 0)
stamps = torch.zeros(16, dtype=torch.int64, device=dev)
lib.paac_debug_set_misc_stamps(ctypes.c_void_p(stamps.data_ptr()))
# ... and the conv tower's own stamps (csrc/tower.h: 12 per wave, [workgroup][wave]; slots 6 -> 7 are phase 2: conv2's GEMM on waves
# 0-3, the kept rows and whatever rides on waves 4-7), left by the last tower launch of each run
lib.paac_debug_set_tower_stamps.argtypes = [ctypes.c_void_p]
tstamps = torch.zeros(12 * 8 * 8 * N, dtype=torch.int64, device=dev)
lib.paac_debug_set_tower_stamps(ctypes.c_void_p(tstamps.data_ptr()))
ctx = hip_ops.Context(1, A, max_batch=N)
params = torch.randn(ctx.layout["total"], device=dev) * 0.02
if os.environ.get("PROBE_KEEP", "0") != "1":      # PROBE_KEEP=1: unmanaged weights -- the acting tower is the kept-rows variant
    ctx.set_managed_weights(True)
    ctx.pack_weights(params)
mt =hip_ops.mt_state_from_numpy(np.random.RandomState(1).get_state(), dev)
stacks = torch.zeros((T + 1, N, 84, 84, 4), dtype=torch.uint8, device=dev)
hip_ops.synth_reset(3, 0, stacks[0], None)
act = torch.zeros((T, N), dtype=torch.int32, device=dev)
val = torch.zeros((T, N), device=dev); rew = torch.zeros((T, N), device=dev); msk = torch.zeros((T, N), device=dev)
probs = torch.zeros((N, A), device=dev)
epr = torch.zeros(N, device=dev); epl = torch.zeros(N, dtype=torch.int32, device=dev)
fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)
tick = torch.zeros(1, dtype=torch.int64, device=dev)
thr = terminal_threshold(0.01)
# stamp slots in the order the workgroup passes them, and what lies between two of them
order = [14, 0, 1, 13, 2, 3, 4, 6, 7, 8]
names = ["entry: requests issued", "loads landed, state words parked", "phase-1 ranges", "phase 1 (hooked: nothing)",
         "phase 2 (state blocks)", "phase 3 (doubles) + heads finish / parked record (stamps 3 -> 4)", "walks", "write-back",
         "bookkeeping"]
reps = 40
acc = np.zeros(len(order) - 1)
tower, fc_first, fc_ridden = [], [], []
phase2, phase3 = [], []
ctx.prof_enable(True)
for r in range(reps + 5):
    torch.cuda.synchronize()
    for t in range(T):
        ctx.act_step_pipe(params, stacks[t], mt, act[t], probs, val[t], 3, 0, thr, tick, t, stacks[t + 1], rew[t], msk[t], epr, epl,
                          fin)
    torch.cuda.synchronize()
    st = stamps.cpu().numpy().astype(np.float64)
    events = ctx.prof_read()
    ctx.act_step_flush()
    torch.cuda.synchronize()
    ctx.prof_read()
    if r < 5:
        continue
    acc += np.diff(st[order])
    ts = tstamps.cpu().numpy().reshape(-1, 8, 12).astype(np.float64)
    phase2.append(ts[:, :, 7] - ts[:, :, 6])
    phase3.append(ts[:, :, 9] - ts[:, :, 8])
    tw = [ms * 1000.0 for name, _, ms in events if name == "conv_tower"]
    fc = [ms * 1000.0 for name, _, ms in events if name == "fc_fwd"]
    tower += tw[1:]
    fc_first.append(fc[0])
    fc_ridden += fc[1:]
total = acc.sum()
for n, v in zip(names, acc / reps):
    print("%-84s %7.2f us  %5.1f %%" % (n, v / 100.0, 100.0 * v * reps / total))
print("%-84s %7.2f us" % ("sampler workgroup, entry -> end", total / reps / 100.0))
print("launch durations, us (medians): tower behind a ridden fc launch %.2f | first fc launch of the run (nothing owed) %.2f | "
      "fc launch with the sampler workgroup %.2f" % (np.median(tower), np.median(fc_first), np.median(fc_ridden)))
p2 = np.median(np.stack(phase2), axis=0)        # [workgroup][wave], cycles
print("tower phase 2 (stamps 6 -> 7), median cycles: workgroup 0 GEMM waves %s | its helper waves %s | workgroup 1 helper waves %s | "
      "all other workgroups: GEMM waves %.0f, helper waves %.0f" % (p2[0, :4].astype(int).tolist(), p2[0, 4:].astype(int).tolist(),
                                                                  p2[1 % len(p2), 4:].astype(int).tolist(), np.median(p2[1:, :4]),
                                                                  np.median(p2[1:, 4:])))
# the workgroups that finish heads (csrc/tower.h: RIDER -- 0 .. 3, wave 4 each) beside one that does not, phase 2 and phase 3
# (stamps 8 -> 9: conv3's GEMM on waves 0-3; the kept conv2 rows and the heads finish on waves 4-7)
p3 = np.median(np.stack(phase3), axis=0)
for w in range(min(5, len(p2))):
    print("workgroup %d: phase 2 GEMM waves %s helper waves %s | phase 3 GEMM waves %s helper waves %s" % (
        w, p2[w, :4].astype(int).tolist(), p2[w, 4:].astype(int).tolist(), p3[w, :4].astype(int).tolist(), p3[w, 4:].astype(int).tolist()))
print("workgroups 4 and up, medians: phase 2 GEMM waves %.0f helper waves %.0f | phase 3 GEMM waves %.0f helper waves %.0f" % (
    np.median(p2[4:, :4]), np.median(p2[4:, 4:]), np.median(p3[4:, :4]), np.median(p3[4:, 4:])))
if hasattr(lib, "paac_act_tower_rode"):
    print("the last tower carried (1 heads finish | 2 frame shift):", lib.paac_act_tower_rode(ctx.handle))
