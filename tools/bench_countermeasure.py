#!/usr/bin/env python
"""Times one training iteration of the spoof countermeasure (zero_grad, forward, loss, backward, optimizer step) at B = 64 on the
reference's two input sizes -- ``lin`` (513 x 400) and ``mel`` (80 x 100) -- for

  hip    ``countermeasure.CmLinDisc / CmMelDisc`` (HIP trunk, fused head ``ops.cm_head``) + ``train.FusedAdamEx``;
  stock  the same model, same weights, on torch's stock ops on the same GPU: fp32, eager, the loss as main_spoof_conv1d.py:87 writes it,
         ``torch.optim.Adam(betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-4, amsgrad=True)``.

Method: random features in [0, 1) and alternating labels, uploaded once.  Both arms run in ONE process and alternate block by block
(``--iters`` iterations per block); a block is timed with device events around it (no host synchronisation inside) and one figure is
block time / iterations; every arm is warmed up by one untimed block first.  Reported: the median over ``--blocks`` blocks with
[fastest .. slowest], and stock / hip.  Dropout is active in both arms (each draws its own masks).

    python tools/bench_countermeasure.py [--blocks 7] [--iters 20] [--out profiles/countermeasure.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"lin": (513, 400), "mel": (80, 100)}


def stock_forward(m, x):
    """The classifier of anti_spoofing/discriminator.py on torch's own ops, from the parameters of the module ``m``."""
    import torch
    import torch.nn.functional as F
    tr = m.training
    ln = lambda t, l: F.layer_norm(t.permute(0, 2, 1), l.normalized_shape, l.weight, l.bias, l.eps).permute(0, 2, 1)
    dp = lambda t: F.dropout(t, 0.05, tr)
    conv = lambda t, c: F.conv1d(t, c.weight, c.bias, padding=c.padding[0], dilation=c.dilation[0])
    x = dp(ln(conv(x, m.conv1), m.ln1))
    h = conv(x, m.hc.conv)
    c = h.shape[1] // 2
    s = torch.sigmoid(ln(h[:, :c], m.hc.ln1))
    x = dp(s * ln(h[:, c:], m.hc.ln2) + (1 - s) * x)
    x = ln(F.avg_pool1d(conv(x, m.conv2), m.pl1.kernel_size[0]), m.ln2)
    x = dp(F.leaky_relu(x, 0.05))
    x = ln(F.avg_pool1d(conv(x, m.conv3), m.pl2.kernel_size[0]), m.ln3)
    x = ln(conv(F.leaky_relu(x, 0.05), m.conv4), m.ln4)
    x = F.adaptive_avg_pool1d(conv(F.leaky_relu(x, 0.05), m.conv5), 1)
    return torch.sigmoid(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "countermeasure.txt"))
    a = ap.parse_args()
    import copy
    import torch
    from spoofsv_amd import countermeasure as C
    from spoofsv_amd.train import FusedAdamEx
    if not torch.cuda.is_available():
        raise SystemExit("bench_countermeasure: needs a ROCm device; a CPU run measures nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("countermeasure training iteration, B = %d, DISC_DIM = %d, %s; %d blocks of %d iterations per arm after one untimed block, arms "
        "alternating, device events; ms per iteration, median [fastest .. slowest]"
        % (a.batch, cfg["DISC_DIM"], torch.cuda.get_device_name(dev), a.blocks, a.iters))
    for feat, (Fb, T) in SHAPES.items():
        torch.manual_seed(0)
        hip = C.build_model(cfg, feat).to(dev).train()
        stock = copy.deepcopy(hip)
        x = torch.rand(a.batch, Fb, T, device=dev)
        y = (torch.arange(a.batch, device=dev) % 2).float()
        opt_h = FusedAdamEx(hip.parameters(), **C.ADAM)
        opt_h.refresh_resident_weights()
        opt_s = torch.optim.Adam(stock.parameters(), **C.ADAM)

        def it_hip():
            opt_h.zero_grad()
            loss, _ = hip.loss(x, y)
            loss.backward()
            opt_h.step()

        def it_stock():
            opt_s.zero_grad()
            pred = stock_forward(stock, x).squeeze()
            loss = (-y * torch.log(pred + 1e-6) - (1 - y) * torch.log(1 - pred + 1e-6)).mean()
            loss.backward()
            opt_s.step()
        arms = {"hip": it_hip, "stock": it_stock}
        times = {k: [] for k in arms}
        for blk in range(a.blocks + 1):
            for k, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if blk:
                    times[k].append(e0.elapsed_time(e1) / a.iters)
        m = {k: med(v) for k, v in times.items()}
        for k in arms:
            say("%s (%d x %d), %-5s: %.3f ms [%.3f .. %.3f]" % (feat, Fb, T, k, m[k][0], m[k][1], m[k][2]))
        say("%s: stock / hip = %.2f" % (feat, m["stock"][0] / m["hip"][0]))
        del hip, stock, opt_h, opt_s
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
