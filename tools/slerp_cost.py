"""Cost of the latent interpolation kernel (ops.slerp, gmk_slerp) and of `GaussianDiffusion.interpolate` around it, at 3x32x32.

    python tools/slerp_cost.py [rounds=7] [launches=50] [ode_steps=4]

  * kernel time (events around `launches` back-to-back launches, median of `rounds`) of gmk_slerp at B = 2048, n = 3072, K = 8 - it reads a and b
    once and writes K frames, (2 + K) B n 4 bytes - against a device-to-device copy that moves the same bytes (a buffer of (2 + K) / 2 B n
    floats: read once, written once);
  * wall time (host clock around a call that ends in a synchronise, median of `rounds`) of `interpolate` on B = 2048 pairs in K = 8 frames on
    `ode_steps` ODE steps against the `encode` of the 2 B images and the `decode`s of the K B latents it contains (the same chunks), on the
    default 16-bit net: what the slerp launch, the time table and the concatenations add to (2 + K) N forwards.
A probe, not a gate: the kernel runs once per call."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from generative_models_amd.diffusion.simple_unet import SimpleUnet  # noqa: E402

B, SHAPE, K = 2048, (3, 32, 32), 8


def kernel_ms(launch, rounds, k):
    times = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            launch()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / k)
    return statistics.median(times)


def wall_ms(fn, rounds):
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def run():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randn((B,) + SHAPE, device="cuda", generator=g)
    b = torch.randn((B,) + SHAPE, device="cuda", generator=g)
    t = torch.tensor([j / (K - 1) for j in range(K)], dtype=torch.float32, device="cuda")
    out = torch.empty((K, B) + SHAPE, device="cuda")
    nbytes = (2 + K) * B * n * 4
    src = torch.randn(((2 + K) * B * n // 2,), device="cuda", generator=g)
    dst = torch.empty_like(src)
    slerp = lambda: ops.check(ops.lib.gmk_slerp(a.data_ptr(), b.data_ptr(), t.data_ptr(), out.data_ptr(), None, B, n, K, ops._s()), "slerp")
    copy = lambda: dst.copy_(src)
    for fn in (slerp, copy):
        kernel_ms(fn, 2, k)
    t_slerp, t_copy = kernel_ms(slerp, rounds, k), kernel_ms(copy, rounds, k)
    print(f"B = {B}, n = {n}, K = {K}: {nbytes / 1e6:.1f} MB per call", flush=True)
    for name, ms in (("gmk_slerp  ", t_slerp), ("device copy", t_copy)):
        print(f"{name}  {ms * 1e3:8.1f} us per call  {nbytes / ms / 1e9:6.2f} TB/s")
    print(f"slerp / copy: {t_slerp / t_copy:.2f}x", flush=True)

    torch.manual_seed(0)
    net = SimpleUnet(128, 0.0, in_channels=SHAPE[0]).cuda().eval()
    d = GaussianDiffusion(mean_type="v", num_steps=N)
    xa, xb = a.clamp(-1, 1), b.clamp(-1, 1)
    guide = torch.full((B,), -1, dtype=torch.long, device="cuda")
    lat = d.interpolate(net=partial(net, guide=guide), xa=xa, xb=xb, frames=K, num_steps=N, return_latents=True)[1]
    per = max(1, d.INTERP_MAX_BATCH // B)

    def whole():
        d.interpolate(net=partial(net, guide=guide), xa=xa, xb=xb, frames=K, num_steps=N)

    def parts():
        d.encode(net=partial(net, guide=guide.repeat(2)), x=torch.cat([xa, xb]), num_steps=N)
        for c in lat.split(per):
            d.decode(net=partial(net, guide=guide.repeat(len(c))), z=c.reshape((-1,) + SHAPE), num_steps=N)
    for fn in (whole, parts):
        wall_ms(fn, 1)
    t_parts, t_whole = wall_ms(parts, rounds), wall_ms(whole, rounds)
    t_parts2, t_whole2 = wall_ms(parts, rounds), wall_ms(whole, rounds)            # alternated: the spread of the same code
    print(f"interpolate, {B} pairs, {K} frames, {N} ODE steps ({N} forwards of {2 * B} images, {K * N} of {per * B}):")
    print(f"  interpolate        {t_whole:9.1f} ms   (again {t_whole2:9.1f})")
    print(f"  encode + decodes   {t_parts:9.1f} ms   (again {t_parts2:9.1f})")
    print(f"interpolate / (encode + decode): {min(t_whole, t_whole2) / min(t_parts, t_parts2):.3f}x")


if __name__ == "__main__":
    run()
