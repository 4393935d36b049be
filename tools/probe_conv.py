#!/usr/bin/env python3
"""Time single conv GEMM launches (forward / dgrad / wgrad) per ResNet-18 layer through the
C-ABI test hooks.  Used with FEDMLP_HIP_LIB=build/probeN/libfedmlp_hip.so timing-only builds
(tools/build_probes.sh) to attribute kernel time; not part of the product."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fedmlp_amd.engine import Engine
from fedmlp_amd import spec

imgs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
layers = [int(a) for a in sys.argv[2].split(",")] if len(sys.argv) > 2 else [0, 1, 6, 11, 16]
ops = [int(a) for a in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0]
model = sys.argv[4] if len(sys.argv) > 4 else "Resnet18"
e = Engine(model, 5, 224, 224, imgs)
flat, cnt = spec.init_state(model, 5, 1037)
e.set_state(flat, cnt)
if layers == [-1]:
    layers = list(range(e.debug_num_convs()))
if ops == [3]:
    # op 3: the grouped input gradient of the stride-2 blocks (one launch: four parity classes + the downsample's gradient);
    # FLOPs = both convs' -- like for like with `op 1` of convs 5 + 7, 10 + 12, 15 + 17
    for b, c1, ds in ((2, 5, 7), (4, 10, 12), (6, 15, 17)):
        i1, i2 = e.debug_conv_info(c1), e.debug_conv_info(ds)
        dy1 = torch.randn((imgs, i1["hout"], i1["wout"], i1["cout_p"]), device="cuda")
        dyd = torch.randn_like(dy1)
        dx = torch.empty((imgs, i1["hin"], i1["win"], i1["cin_p"]), device="cuda")
        flops = 2.0 * i1["hout"] * i1["wout"] * i1["cout"] * i1["cin"] * (i1["k"] ** 2 + i2["k"] ** 2) * imgs
        for _ in range(3):
            e.debug_block_dgrad(b, dy1, dyd, dx, imgs)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 10
        t0.record()
        for _ in range(n):
            e.debug_block_dgrad(b, dy1, dyd, dx, imgs)
        t1.record(); torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / n
        print(f"block{b} grouped dgrad (convs {c1} + {ds}, two plane splits included): {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TF", flush=True)
    sys.exit(0)
for ci in layers:
    info = e.debug_conv_info(ci)
    x = torch.randn((imgs, info["hin"], info["win"], info["cin_p"]), device="cuda")
    dy = torch.randn((imgs, info["hout"], info["wout"], info["cout_p"]), device="cuda")
    outs = {0: torch.empty_like(dy), 1: torch.empty((imgs, info["hin"], info["win"], info["cin_p"]), device="cuda"),
            2: torch.empty((info["cout_p"], info["Kw"]), device="cuda")}
    gb = 4e-9 * imgs * (info["hin"] * info["win"] * info["cin_p"] + info["hout"] * info["wout"] * info["cout_p"])
    flops = 2.0 * info["hout"] * info["wout"] * info["cout"] * info["cin"] * info["k"] ** 2 * imgs
    for op in ops:
        # op 1 on the stem (cin 3) is the input-gradient kernel of fm_backward_grads_x (stem_dgrad.hip): dy alone, so that the
        # framing of x the hook does for the packed stem stays out of the time
        xin = None if op == 1 else x
        for _ in range(3):
            e.debug_conv(op, ci, xin, dy, outs[op], imgs)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 10
        t0.record()
        for _ in range(n):
            e.debug_conv(op, ci, xin, dy, outs[op], imgs)
        t1.record(); torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / n
        print(f"conv{ci:2d} op{op} cin{info['cin']:4d} cout{info['cout']:4d} k{info['k']} s{info['stride']} "
              f"hout{info['hout']:4d}: {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TF  {gb/ms:6.2f} TB/s (x+y once)", flush=True)
