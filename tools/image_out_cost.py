"""What turning samples into bytes and pictures costs, against the torch chain evaluate() used before gmk_to_uint8 existed.

    python tools/image_out_cost.py [out=profiles/image_out_cost.txt]

  (1) quantise   a [1000, 25, 3, 32, 32] fp32 trajectory (307 MB) -> uint8 on the device: ops.to_uint8 (one launch) against the chain
                 ((t + 1) * 127.5).clamp(0, 255).to(torch.uint8) on the same tensor, interleaved; time from device events, and the peak of
                 torch.cuda.max_memory_allocated above what was allocated before the call.
  (2) evaluate   DiffusionModel.evaluate() at 3 x 32 x 32, timesteps 250, hidden_size 128, three arms on one model, interleaved:
                 (a) NullWriter with that torch chain in place of ops.to_uint8 (the chain and its .cpu(), as before), (b) NullWriter,
                 (c) ImageWriter (1 PNG + 3 APNGs of 60 frames).  For (c) the host time inside pngio's encoders (zlib's deflate and the chunk
                 framing) is taken apart from the rest (sampling, kernels, copies to the host).
Each part runs in a child process of its own under a time limit; a part that fails ends the run."""
import statistics
import subprocess
import sys
import tempfile
import time

PARTS = {"quantise": 240, "evaluate": 420}          # seconds a part may take


def torch_chain(t, crop=0):
    import torch
    t = ((t + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    return t[..., crop:t.shape[-2] - crop, crop:t.shape[-1] - crop] if crop else t


def quantise(emit):
    import torch
    from generative_models_amd import ops
    shape = (1000, 25, 3, 32, 32)
    x = torch.empty(shape, device="cuda").uniform_(-1.2, 1.2)
    emit(f"# {torch.cuda.get_device_name(0)}")
    emit(f"(1) quantise {list(shape)} fp32 = {x.numel() * 4 / 1e6:.0f} MB -> uint8 {x.numel() / 1e6:.0f} MB")
    arms = {"torch chain": torch_chain, "ops.to_uint8": ops.to_uint8}
    assert torch.equal(arms["torch chain"](x), arms["ops.to_uint8"](x))
    emit("  both arms give the same bytes")
    times, peaks = {k: [] for k in arms}, {}
    for name, fn in arms.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn(x)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out
    for r in range(20):
        for name in (list(arms) if r % 2 == 0 else reversed(list(arms))):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            arms[name](x)
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3)
    moved = x.numel() * 5
    for name in arms:
        med = statistics.median(times[name])
        emit(f"  {name:13s}: median {med:8.1f} us of 20 (min {min(times[name]):.1f}), {moved / med / 1e6:.2f} TB/s of the {moved / 1e6:.0f} MB one pass "
             f"moves; peak allocation above the input {peaks[name] / 1e6:7.1f} MB")
    a, b = statistics.median(times["torch chain"]), statistics.median(times["ops.to_uint8"])
    emit(f"  ops.to_uint8 / torch chain: time {b / a:.2f}x, peak memory {peaks['ops.to_uint8'] / peaks['torch chain']:.2f}x")


def evaluate(emit):
    import torch
    from generative_models_amd import common, ops, pngio
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=250, bs=64, hidden_size=128, in_channels=3, image_size=32)
    torch.manual_seed(0)
    model = Model(G).to("cuda")
    model.eval()
    x = torch.rand(25, 3, 32, 32, device="cuda") * 2 - 1
    y = torch.arange(25, device="cuda") % 10
    host = [0.0]

    def timed(fn):
        def run(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            host[0] += time.perf_counter() - t0
            return out
        return run

    pngio.encode_png, pngio.encode_apng = timed(pngio.encode_png), timed(pngio.encode_apng)
    kernel = ops.to_uint8
    logdir = tempfile.mkdtemp()
    arms = {"(a) NullWriter, torch chain": (torch_chain, common.NullWriter()), "(b) NullWriter": (kernel, common.NullWriter()),
            "(c) ImageWriter": (kernel, common.ImageWriter(logdir))}

    def run(arm):
        ops.to_uint8, writer = arms[arm]
        host[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.evaluate(writer, x, y, 0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, host[0]

    emit("(2) evaluate() at 3 x 32 x 32, timesteps 250, hidden_size 128: seconds per call, 5 rounds, order alternating")
    for arm in arms:
        run(arm)                                     # warm-up
    total, deflate = {a: [] for a in arms}, {a: [] for a in arms}
    for r in range(5):
        for arm in (list(arms) if r % 2 == 0 else reversed(list(arms))):
            t, h = run(arm)
            total[arm].append(t)
            deflate[arm].append(h)
    ops.to_uint8 = kernel
    med = {a: statistics.median(v) for a, v in total.items()}
    for arm in arms:
        h = statistics.median(deflate[arm])
        emit(f"  {arm:28s}: median {med[arm]:.3f} s (spread {(max(total[arm]) - min(total[arm])) / med[arm]:.1%}); in pngio's encoders {h:.3f} s, "
             f"everything else {med[arm] - h:.3f} s")
    emit(f"  (b) - (a): {med['(b) NullWriter'] - med['(a) NullWriter, torch chain']:+.3f} s;  (c) - (b): "
         f"{med['(c) ImageWriter'] - med['(b) NullWriter']:+.3f} s, of which deflate {statistics.median(deflate['(c) ImageWriter']):.3f} s")
    import os
    sizes = {p: os.path.getsize(os.path.join(logdir, "images", p)) for p in sorted(os.listdir(os.path.join(logdir, "images")))}
    emit("  files: " + ", ".join(f"{p} {s / 1e3:.0f} kB" for p, s in sizes.items()))


def main_():
    if len(sys.argv) > 2 and sys.argv[1] == "--part":
        sys.path.insert(0, ".")
        {"quantise": quantise, "evaluate": evaluate}[sys.argv[2]](lambda s: print(s, flush=True))
        return
    out = sys.argv[1] if len(sys.argv) > 1 else "profiles/image_out_cost.txt"
    lines = ["$ python tools/image_out_cost.py"]
    for part, limit in PARTS.items():
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--part", part], capture_output=True, text=True)
        print(done.stdout, end="", flush=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:
            print(done.stderr[-3000:], file=sys.stderr)
            sys.exit(f"part {part!r} ended with status {done.returncode}: nothing further is started")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main_()
