"""Cost of the arena digest (ops.arena_digest, checkpoint.py) and of writing the train state, on the 3x32x32 net (BASELINE configs[2]).

    python tools/digest_cost.py [rounds=7] [launches=50]

  * kernel time (events around `launches` back-to-back launches, median of `rounds`) of gmk_arena_digest over the parameter arena against
    gmk_grad_norm over the same bytes - the project's existing one-read reduction (two launches: partials, then one workgroup);
  * wall time of ops.arena_digest as checkpoint.py calls it (launch + the 8-byte read-back, a host sync);
  * wall time of Session.checkpoint with --save_state 0 and 1 (eval_heavy 0: the weights file, then the state file with Adam's two moments
    and four digests), after one train step so that the moments exist.
The digest runs once per checkpoint; it has no time bar.  Each of its words costs two 64-bit multiplies (four 32-bit multiply pairs each on this
hardware) where the norm costs one fused multiply-add."""
import contextlib
import io
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import main, ops  # noqa: E402
from generative_models_amd._lib import check, lib  # noqa: E402


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


def session(logdir, save_state):
    argv = ["--model=diffusion", "--in_channels", "3", "--image_size", "32", "--bs", "32", "--eval_heavy", "0", "--logdir", logdir,
            "--save_state", str(save_state)]
    torch.manual_seed(0)
    s = main.Session(*main.load_model_and_data(argv))
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((32, 3, 32, 32), generator=g) * 2 - 1).cuda()
    s.model.train()
    s.model.train_step(x, torch.randint(0, 10, (32,), generator=g).cuda())
    return s


def run():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    with tempfile.TemporaryDirectory() as tmp:
        sessions = {flag: session(f"{tmp}/state{flag}", flag) for flag in (0, 1)}
        net = sessions[1].model.net
        p = net.flat_params
        n = p.numel()
        print(f"3x32x32 net: arena of {n} floats, {4 * n / 1e6:.1f} MB per read", flush=True)
        out = torch.empty((1,), dtype=torch.int64, device=p.device)
        state = torch.zeros(4, dtype=torch.float32, device=p.device)
        ws = ops.grad_norm_workspace(n, p.device)
        digest = lambda: check(lib.gmk_arena_digest(p.data_ptr(), n, out.data_ptr(), ops._s()), "arena_digest")
        norm = lambda: ops.grad_norm(p, state, 1.0, 0.0, ws)
        for fn in (digest, norm):
            kernel_ms(fn, 2, k)
        t_digest, t_norm = kernel_ms(digest, rounds, k), kernel_ms(norm, rounds, k)
        for name, t in (("gmk_arena_digest", t_digest), ("gmk_grad_norm   ", t_norm)):
            print(f"{name}  {t * 1e3:8.1f} us per call  {4 * n / t / 1e6:8.1f} GB/s read")
        print(f"digest / grad_norm: {t_digest / t_norm:.2f}x")
        print(f"ops.arena_digest (launch + read-back of the value): {wall_ms(lambda: ops.arena_digest(p), rounds) * 1e3:.1f} us wall")
        for flag, s in sessions.items():
            log = main.EpochLog("diffusion")
            with contextlib.redirect_stdout(io.StringIO()):             # "SAVED MODEL ..." per call
                s.checkpoint(log, (None, None), 0)
                t = wall_ms(lambda: s.checkpoint(log, (None, None), 0), rounds)
            print(f"Session.checkpoint, --save_state {flag}: {t:.1f} ms wall")


if __name__ == "__main__":
    run()
