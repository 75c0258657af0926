"""Decode loop of the Qwen3-8B-shaped model as an MLX checkpoint (for rocprofv3 / quick timing):
quant_decode.py [bits (4; 0 = bf16)] [ctx] [--recipe mixed_2_6|mixed_3_4|mixed_3_6|mixed_4_6] [--windows N].
--recipe: a mixed-precision checkpoint with synthetic weights -- v_proj / down_proj of the recipe's layers and lm_head at the wide
format, everything else narrow, group 64 (engine.mixed_recipe: the layer rule is written down from memory of mlx_lm and marked so
there).
--windows N: N timed windows of 64 steps in this process (the spread between them is the noise floor of an A/B)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import
omx = omx_import.load_package()
from ominix_mlx_amd import engine
argv = list(sys.argv[1:])


def take(flag, dflt):
    if flag in argv:
        i = argv.index(flag)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return dflt


recipe = take("--recipe", None)
windows = int(take("--windows", 1))
bits = int(argv[0]) if len(argv) > 0 else 4
ctx = int(argv[1]) if len(argv) > 1 else 2048
L = 36
quant = {"bits": bits, "group_size": 64} if bits else None
label = f"bits {bits}"
if recipe:
    quant = engine.mixed_recipe_quantization(recipe, L)
    label = recipe
m = engine.Model(hidden_size=4096, num_hidden_layers=L, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                 head_dim=128, vocab_size=151936, max_context=ctx + 200 + 64 * windows, quantization=quant)
m.synth_weights()
m.prefill(((np.arange(ctx, dtype=np.uint32) * 7919) + 13) % 151936)
m.decode(8)
for w in range(windows):
    t0 = time.perf_counter(); m.decode(64); dt = time.perf_counter() - t0
    print(f"{label} ctx {ctx}: {64/dt:.1f} tok/s  {dt/64*1e3:.3f} ms/step  device {m.last_decode_ms()/64:.3f} ms  "
          f"{m.step_bytes(ctx) / 1e9:.3f} GB/token", flush=True)
m.close()
