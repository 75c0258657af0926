"""The grouped read of forked slots against the rows' own blocks, at Qwen3-8B shapes in bf16:

    python tools/batch_fork_sweep.py [--ctx 2048 8192] [--steps 128] [--windows 3]
        one process, one model: per prompt length, 8 / 4 / 2 slots forked from one prompt, decoded with OMX_BATCH_SHARE=0 (every row
        on its own slab) and with grouped blocks from two members on (OMX_BATCH_SHARE_MIN=2) at 8 / 4 / 2 / 1 member rows per block
        (OMX_BATCH_SHARE_ROWS); the switches are set before each Model.batch, which reads them.  tools/batch_decode.py's protocol:
        median of --windows windows of --steps steps after 8 warm-up steps, device events.  One JSON line per run;
        tokens_equal_share_off says whether the run's tokens are those of the OMX_BATCH_SHARE=0 run of the same row."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--ctx", type=int, nargs="+", default=[2048, 8192])
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--layers", type=int, default=36)
args = ap.parse_args()

import omx_import
omx_import.load_package()
from ominix_mlx_amd import engine

V = 151936
room = 8 + args.steps * args.windows + 16
m = engine.Model(hidden_size=4096, num_hidden_layers=args.layers, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                 head_dim=128, vocab_size=V, max_context=max(args.ctx) + room)
m.synth_weights()
os.environ["OMX_BATCH_SHARE_MIN"] = "2"
for ctx in args.ctx:
    prompt = ((np.arange(ctx, dtype=np.int64) * 7919 + 13) % V).astype(np.uint32)
    for siblings, forms in [(8, [None, 8, 4, 2, 1]), (4, [None, 4, 2, 1]), (2, [None, 2, 1])]:
        ref = None
        for rows in forms:
            os.environ["OMX_BATCH_SHARE"] = "0" if rows is None else "1"
            os.environ["OMX_BATCH_SHARE_ROWS"] = str(rows or 8)
            b = m.batch(8, ctx + room)
            b.prefill(0, prompt)
            for s in range(1, siblings):
                b.set_sampler(s, 0.8, s)
                b.fork(0, s)
            slots = list(range(siblings))
            b.decode(8, slots)
            ms, toks = [], []
            for _ in range(args.windows):
                toks.append(b.decode(args.steps, slots))
                ms.append(b.last_decode_ms() / args.steps)
            toks = np.concatenate(toks)
            ref = toks if ref is None else ref
            print(json.dumps({"ctx": ctx, "siblings": siblings, "rows_per_block": rows or "own blocks (OMX_BATCH_SHARE=0)",
                              "shared_len": b.shared(1)[1], "ms_per_step": float(np.median(ms)), "windows_ms": ms,
                              "tokens_equal_share_off": bool((toks == ref).all())}), flush=True)
            b.close()
m.close()
