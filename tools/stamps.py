"""Per-phase cycle stamps of the fused MLP kernels (diagnostics build: make EXTRA=-DNERF_STAMPS), wave 0 of workgroup 0.

    python tools/stamps.py [fp32|f16x3] [rgbskip]

Without `rgbskip`: model_predict, i.e. the full kernel.  With it (f16x3 only): a render_rays call that reads rgb alone, i.e.
mlp_f16x3_rgbskip_kernel -- twice, with the sigma head's bias at -50 (every tile skipped) and at +1.5 (none skipped) -- whose
vote and fast-forward phases then stand next to the prologue.  (tools/rgb_skip_measure.py writes the same table to a file.)"""
import os, sys, ctypes, numpy as np
sys.path.insert(0, os.getcwd())
import nerf_and_dietnerf_amd as N
prec = sys.argv[1] if len(sys.argv) > 1 else "fp32"
rgbskip = len(sys.argv) > 2 and sys.argv[2] == "rgbskip"
names = ["prologue","L0(PE)","HID x6","L4(SKIP)","L8(LAST)","heads","tiles","vote","skip: store+ff","skipped tiles"]
ideal = [0, 136*64, 6*1024*64, 1160*64, 560*64, 0] if prec == "fp32" else [0, 72*32, 6*384*32, 456*32, 270*32, 0]


def table():
    out = (ctypes.c_ulonglong*16)()
    (N._lib.load().nerf_debug_read_stamps if prec == 'fp32' else N._lib.load().nerf_debug_read_stamps_h)(out)
    v = list(out)[:10] if prec != "fp32" else list(out)[:8] + [0, 0]
    nt = v[6]
    for n,x,i in zip(names, v, ideal+[0, 0, 0, 0]):
        if n in ("tiles", "skipped tiles"):
            print(f"{n:14s} {x:12d}")
        else:
            print(f"{n:14s} {x/ max(nt,1):12.0f} cyc/tile  ideal {i}  eff {i/(x/nt) if x and i else 0:.3f}")
    tot = (sum(v[:6]) + v[7] + v[8]) / nt
    print("total/tile", tot, "ideal", sum(ideal), "eff", sum(ideal)/tot)


M = 128*256*64   # 64 tiles per workgroup
rng = np.random.default_rng(0)
if not rgbskip:
    ctx = N.Context(near=2/3, far=5/3, precision=prec)
    ctx.load_weights(0, N.glorot_blob(0))
    xyz = rng.uniform(-1,1,(M,3)).astype(np.float32); d = rng.uniform(-1,1,(M,3)).astype(np.float32)
    ctx.model_predict(0, xyz, d)
    ctx.enable_timing(True)
    ctx.model_predict(0, xyz, d)
    ms, nl, rows = ctx.read_timing()
    print(f'wall: {ms:.3f} ms for {rows} rows -> {rows*1024304/ms/1e9:.1f} TFLOP/s algorithmic')
    table()
else:
    n, s = M // 64, 64
    o = np.zeros((n, 4), np.float32); o[:, :3] = rng.uniform(-0.3, 0.3, (n, 3)); o[:, 2] += 1.5
    d = np.zeros((n, 4), np.float32); d[:, :3] = rng.uniform(-0.4, 0.4, (n, 3)); d[:, 2] = -1.0
    z = np.sort(rng.uniform(2/3, 5/3, (n, s)), axis=1).astype(np.float32)
    rgb = np.empty((n, 3), np.float32)
    for bias in (-50.0, 1.5):
        blob = N.glorot_blob(1); blob[-1] = bias
        ctx = N.Context(near=2/3, far=5/3, precision="f16x3")      # a fresh context: the per-launch gate knows nothing yet
        ctx.load_weights(0, blob)
        outs = N._lib.NerfOutputs(); outs.rgb = rgb.ctypes.data
        N._lib.check(ctx.lib.nerf_render_rays(ctx.h, 0, o.ctypes.data, d.ctypes.data, z.ctypes.data, n, s, ctypes.byref(outs),
                                              N._lib.NERF_MEM_HOST))
        print(f"--- rgb-skipping kernel, sigma bias {bias}")
        table()
        ctx.close()
