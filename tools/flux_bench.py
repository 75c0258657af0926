"""FLUX.2-klein denoise-step timing on one MI355X (BASELINE config 5 at TP=1): full-size model
(3072 hidden, 24 heads, 5 double + 20 single blocks), synthetic weights/inputs, bf16.
    python tools/flux_bench.py [res]                   the bf16 step
    python tools/flux_bench.py [res] --bits [4,8]      bf16, then the quantized DiT (klein.FluxKlein.quantize, group 64) at each width,
                                                       each also with OMX_KLEIN_QGEMM=0 (dequantise into scratch + bf16 GEMM): one
                                                       process, one model at a time, weight_bytes() of each"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import omx_import
omx = omx_import.load_package()
from ominix_mlx_amd import klein

def run(res=1024, s_txt=512, steps=4, warmup=1, bits=0, group=64, m=None):
    g = res // 16
    s_img = g * g
    own = m is None
    if own:
        m = klein.FluxKlein()
        m.synth_weights()
        if bits:
            m.quantize(group, bits)
    lat = omx.ops.fill_uniform((s_img, 128), 1, 1.7)
    txt = omx.ops.fill_uniform((s_txt, 7680), 2, 1.7)
    rc, rs = klein.compute_rope(klein.create_txt_ids(s_txt), klein.create_img_ids(g, g))
    for _ in range(warmup):
        m.forward_with_rope(lat, txt, 1000.0, rc, rs)
    ts = []
    for i in range(steps):
        t = 1.0 - i / steps
        m.forward_with_rope(lat, txt, t * 1000.0, rc, rs)
        ts.append(m.last_ms())
    S = s_txt + s_img
    h, mh = 3072, 9216
    lin = 2 * (s_img * 128 * h + s_txt * 7680 * h + 5 * 2 * 0 + 0)  # embedders
    lin += 5 * (2 * S * (4 * h * h) + 2 * S * (h * 2 * mh) + 2 * S * (mh * h))
    lin += 20 * (2 * S * h * (3 * h + 2 * mh) + 2 * S * (h + mh) * h)
    lin += 2 * s_img * h * 128
    attn = 25 * 4 * S * S * h
    flop = lin + attn
    ms = float(np.median(ts))
    dt = f"int{bits} g{group}" if bits else "bf16"
    out = {"workload": f"flux.2-klein {res}x{res} {dt}, S_img={s_img}, S_txt={s_txt}", "sec_per_step": round(ms / 1e3, 5),
           "ms_all": [round(t, 2) for t in ts], "tflop_per_step": round(flop / 1e12, 2),
           "achieved_tflops": round(flop / ms / 1e9, 1), "mfma_frac_of_2500": round(flop / ms / 1e9 / 2500.0, 4)}
    if bits:
        out["qgemm"] = os.environ.get("OMX_KLEIN_QGEMM", "1") != "0"
    out["weight_bytes"] = m.weight_bytes()
    if own:
        m.close()
    return out

def run_bits(res, widths):
    rows = [run(res)]
    base = rows[0]["sec_per_step"]
    for bits in widths:
        m = klein.FluxKlein()
        m.synth_weights()
        m.quantize(64, bits)
        for qg in ("1", "0"):
            os.environ["OMX_KLEIN_QGEMM"] = qg
            r = run(res, bits=bits, m=m)
            r["step_vs_bf16"] = round(r["sec_per_step"] / base, 3)
            r["bytes_vs_bf16"] = round(r["weight_bytes"] / rows[0]["weight_bytes"], 3)
            rows.append(r)
        os.environ.pop("OMX_KLEIN_QGEMM", None)
        m.close()
    return rows

if __name__ == "__main__":
    args = sys.argv[1:]
    widths = None
    if "--bits" in args:
        i = args.index("--bits")
        val = args[i + 1] if i + 1 < len(args) else ""
        given = bool(val) and all(b in ("4", "8") for b in val.split(","))
        widths = [int(b) for b in val.split(",")] if given else [8, 4]
        del args[i:i + (2 if given else 1)]
    res = int(args[0]) if args else 1024
    if widths is None:
        print(json.dumps(run(res)), flush=True)
    else:
        for r in run_bits(res, widths):
            print(json.dumps(r), flush=True)
