"""Timeline of the decode-step attention kernel (csrc/attn_step.hip) on Qwen3-8B shapes: one eager step with the
kernel's wall-clock stamps on (100 MHz), reported relative to the first block start of each layer's launch.
usage: python tools/attn_step_trace.py [ctx] [layers]"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import
omx = omx_import.load_package()
from ominix_mlx_amd import engine
lib = omx.lib
ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
L = int(sys.argv[2]) if len(sys.argv) > 2 else 12
H = 32
m = engine.Model(hidden_size=4096, num_hidden_layers=L, intermediate_size=12288, num_attention_heads=H,
                 num_key_value_heads=8, head_dim=128, vocab_size=151936, max_context=ctx + 256)
m.synth_weights()
m.prefill((np.arange(ctx, dtype=np.uint32) * 7919) % 151936)
m.decode(8)
W = 16   # trace words per block (csrc/attn.hpp kAttnTraceWords)
buf = np.zeros(L * 64 * 8 * W, np.uint64)
nb = ctypes.c_int()
omx.check(lib.omx_qwen3_debug_trace_step(m._h, buf.ctypes.data, buf.size, ctypes.byref(nb)))
nb = nb.value
t = buf[:L * nb * W].reshape(L, nb, W).astype(np.int64)
names = ["block start", "loads landed, q/k normed+roped", "own chunk done", "granules stored", "gather + merge done (consumers)",
         "attention vector swept into LDS (O projection)", "O rows stored", "all waves' partials parked in LDS (block barrier)"]
# gate/up inside the launch (OMX_ATTN_GATEUP): stamp 7 marks the first reduced (gate, up) pair of wave 0 -- the sweeping wave, whose pair
# is asked for last -- and stamp 4 of an O block (blocks past the first H: the consumers come first) the hidden row swept into LDS.
# Hop three is hidden when "first pair reduced" follows "hidden row swept" by less than a weight round trip.
# Stamps 8 and 9: wave 0 and wave 7 done with their last pair (the pairs are drawn from a ticket counter in the block: the two end
# together); word 10 is a count, not a stamp: the pairs the block's waves reduced (48).
# down + the next layer's q/k/v inside the launch as well (OMX_ATTN_DOWN, layers 0 .. L-2): stamp 11 the activation vector swept into
# LDS (hop four), 12 the first down unit of wave 0 -- the sweeping wave -- reduced, 13 the residual row swept (hop five), 14 the block's
# q/k/v rows stored; word 15 is a count: the down units the block reduced (32) | the q/k/v rows it stored (24) << 32.
gateup = m.step_forms()["attn_gateup"]
down = m.step_forms()["attn_down"]
n_cons = H   # consumer blocks: one per query head, the launch's first blocks
events = [(ev, nm, slice(None)) for ev, nm in enumerate(names)]
if gateup:
    events[4] = (4, names[4], slice(0, n_cons))
    events[7] = (7, "gate/up: first pair reduced (wave 0)", slice(None))
    events.insert(7, (4, "gate/up: hidden row swept into LDS (O blocks)", slice(n_cons, None)))
    events.append((8, "gate/up: last pair of wave 0 reduced", slice(None)))
    events.append((9, "gate/up: last pair of wave 7 reduced", slice(None)))
if down:
    events.append((11, "down: activation vector swept into LDS", slice(None)))
    events.append((12, "down: first unit reduced (wave 0)", slice(None)))
    events.append((13, "q/k/v: residual row swept into LDS", slice(None)))
    events.append((14, "q/k/v: rows stored", slice(None)))
print(f"{nb} blocks per launch, {L} layers, ctx {ctx}, gate/up in the launch: {gateup}, down + next q/k/v in the launch: {down}")
for ev, nm, blocks in events:
    rows = []
    for l in range(1, L - 1 if ev >= 11 else L):
        t0 = t[l, :, 0][t[l, :, 0] > 0].min()
        v = t[l, blocks, ev]
        v = v[v > 0]
        if v.size:
            rows.append(((v - t0) / 100.0))
    if rows:
        allv = np.concatenate(rows)
        print(f"  {nm:48s} median {np.median(allv):6.2f} us   p90 {np.percentile(allv, 90):6.2f}   max(median over layers) "
              f"{np.median([r.max() for r in rows]):6.2f}   n/layer {allv.size // len(rows)}")
if gateup:
    tail = (t[1:, :, 8] - t[1:, :, 9]) / 100.0
    print(f"  wave 0 behind wave 7 at the end of a block: median {np.median(tail):6.2f} us   p90 {np.percentile(tail, 90):6.2f}   "
          f"max {tail.max():6.2f}")
    print(f"  pairs reduced per block: min {t[:, :, 10].min()}   max {t[:, :, 10].max()}")
if down:
    u, r = t[:L - 1, :, 15] & 0xFFFFFFFF, t[:L - 1, :, 15] >> 32
    print(f"  down units reduced per block: min {u.min()}   max {u.max()};   q/k/v rows stored per block: min {r.min()}   max {r.max()}")
m.close()
