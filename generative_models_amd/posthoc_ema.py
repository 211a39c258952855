"""Post-hoc EMA (an extension; Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3.2 and
appendix C): the weights of ANY averaging length from one training run.

During training `--ema_sigma_rel s1[,s2[,s3]]` keeps one power-function average of the weights per width inside the fused Adam launch
(diffusion/optim.py, gmk_adam_pema_step) and writes them to `<logdir>/ema_snapshots/step_<t>.pt` every `--ema_snapshot_every` steps and at
every checkpoint.  Afterwards the average of another width is a least-squares combination of the stored ones:

    python -m generative_models_amd.posthoc_ema --run <logdir> --sigma_rel 0.07 [--at_step t] [--out <file>]
    python -m generative_models_amd.posthoc_ema --run <logdir> --sigma_rel 0.07 --sweep 0.03,0.05,0.07,0.1,0.15 --sweep_batches 4

The first writes `<logdir>/model_ema_0.07.pt`, a state dict `--weights_from` loads; `--sweep` also evaluates `model.loss` on the first test
batches for every listed width and for the online weights (same images, times and noise for every row) into `<logdir>/ema_sweep.csv`.

Definitions.  An average of relative width sigma_rel in (0, 0.2887) has the exponent gamma >= 0 with
sigma_rel = sqrt(gamma + 1) / ((gamma + 2) sqrt(gamma + 3)); after optimiser step t = 1, 2, ... it is e(t) = beta e(t - 1) + (1 - beta) theta(t),
beta = (1 - 1/t)^(gamma + 1): beta = 0 at t = 1, so the average starts as a copy of the first updated weights and its weights over
theta(1 .. t) sum to 1.  Read at step t its continuous profile is p(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t], whose inner
products are closed-form (`profile_dot`); the combination x solves A x = b with A_ij = <p_i, p_j>, b_i = <p_i, p*>.

Everything above `reconstruct` is pure Python / NumPy and imports without the HIP library.  Multi-GPU runs are untested: rank 0 writes the
snapshots of its own replica."""
import argparse
import csv
import itertools
import math
import os
import re
from pathlib import Path

import numpy as np

SIGMA_REL_SUP = 1.0 / math.sqrt(12.0)      # sigma_rel of gamma = 0, the widest power-function average
SIGMA_REL_MIN, SIGMA_REL_MAX = 0.01, 0.25  # what --ema_sigma_rel tracks
MAX_TRACKED = 3                            # averages one optimiser launch updates (gmk_adam_pema_step)
MAX_ARENAS = 64                            # arenas one reconstruction combines (gmk_arena_combine)
RANGE_FACTOR = 1.5                         # a target width may leave the tracked range by this factor on each side
SNAPSHOT_DIR = "ema_snapshots"
SWEEP_FILE = "ema_sweep.csv"


def sigma_rel_from_gamma(gamma):
    gamma = float(gamma)
    if not gamma >= 0.0:
        raise ValueError(f"gamma = {gamma}: a power-function average has gamma >= 0")
    return math.sqrt(gamma + 1.0) / ((gamma + 2.0) * math.sqrt(gamma + 3.0))


def gamma_from_sigma_rel(sigma_rel):
    """The root gamma >= 0 of sigma_rel_from_gamma(gamma) = sigma_rel, by bisection in double (the function decreases monotonically)."""
    s = float(sigma_rel)
    if not 0.0 < s < SIGMA_REL_SUP:
        raise ValueError(f"sigma_rel = {sigma_rel}: a relative width lies in (0, {SIGMA_REL_SUP:.4f})")
    lo, hi = 0.0, 1.0
    while sigma_rel_from_gamma(hi) > s:
        lo, hi = hi, hi * 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if sigma_rel_from_gamma(mid) > s:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def power_weight(gamma, t):
    """w = 1 - beta of the update after optimiser step t >= 1, beta = (1 - 1/t)^(gamma + 1), in double: 1 at t = 1, decreasing in t."""
    t = int(t)
    if t < 1:
        raise ValueError(f"t = {t}: optimiser steps count from 1")
    if t == 1:
        return 1.0
    return -math.expm1((float(gamma) + 1.0) * math.log1p(-1.0 / t))


def profile_dot(ga, ta, gb, tb):
    """<p_a, p_b> of two continuous profiles, in the log domain (t^(gamma + 1) overflows a double):
    (ga + 1)(gb + 1) m^(ga + gb + 1) / ((ga + gb + 1) ta^(ga + 1) tb^(gb + 1)), m = min(ta, tb), with m's powers cancelled by hand."""
    ga, ta, gb, tb = float(ga), float(ta), float(gb), float(tb)
    if not (ta > 0.0 and tb > 0.0 and ga >= 0.0 and gb >= 0.0):
        raise ValueError(f"profile_dot({ga}, {ta}, {gb}, {tb}): t > 0 and gamma >= 0")
    if ta > tb:
        ga, ta, gb, tb = gb, tb, ga, ta
    # ta <= tb: ta^(ga + gb + 1) / (ta^(ga + 1) tb^(gb + 1)) = (ta / tb)^(gb + 1) / ta
    return math.exp(math.log((ga + 1.0) * (gb + 1.0) / (ga + gb + 1.0)) + (gb + 1.0) * math.log(ta / tb) - math.log(ta))


def _gram(snapshots, gamma, t):
    snaps = [(float(g), float(s)) for g, s in snapshots]
    if not snaps:
        raise ValueError("no snapshots to combine")
    K = len(snaps)
    A = np.empty((K, K), dtype=np.float64)
    for i in range(K):
        for j in range(i, K):
            A[i, j] = A[j, i] = profile_dot(*snaps[i], *snaps[j])
    b = np.array([profile_dot(g, s, gamma, t) for g, s in snaps], dtype=np.float64)
    return A, b, profile_dot(gamma, t, gamma, t)


def solve_weights(snapshots, gamma, t):
    """The coefficients x (float64 [K]) with sum_i x_i p_i the least-squares fit of the profile of (gamma, t); snapshots: K pairs
    (gamma_i, t_i).  The profiles are scaled to unit norm first; lstsq, since duplicate snapshots make the Gram matrix singular."""
    A, b, _ = _gram(snapshots, gamma, t)
    d = 1.0 / np.sqrt(np.diag(A))
    y = np.linalg.lstsq(A * d[:, None] * d[None, :], b * d, rcond=None)[0]
    return y * d


def fit_residual(snapshots, gamma, t, x=None):
    """||p* - sum_i x_i p_i||_2 / ||p*||_2 from the Gram quantities alone (x: solve_weights' by default); its floor is about 1e-8, the root of
    the rounding of the three terms it cancels."""
    A, b, c = _gram(snapshots, gamma, t)
    x = solve_weights(snapshots, gamma, t) if x is None else np.asarray(x, dtype=np.float64)
    return math.sqrt(max(0.0, c - 2.0 * float(x @ b) + float(x @ A @ x)) / c)


def parse_sigma_rel(text):
    """'' -> (); '0.05,0.1' (or a sequence of numbers) -> (0.05, 0.1): one to three widths, strictly increasing, each in [0.01, 0.25]."""
    if text is None or (isinstance(text, (str, tuple, list)) and len(text) == 0) or (isinstance(text, str) and text.strip() == ""):
        return ()
    parts = text.split(",") if isinstance(text, str) else list(text)
    try:
        widths = tuple(float(p) for p in parts)
    except (TypeError, ValueError):
        raise ValueError(f"ema_sigma_rel = {text!r}: comma-separated relative widths, e.g. 0.05,0.1") from None
    if not 1 <= len(widths) <= MAX_TRACKED:
        raise ValueError(f"ema_sigma_rel = {text!r}: one to {MAX_TRACKED} widths (one optimiser launch updates at most {MAX_TRACKED} averages)")
    for w in widths:
        if not SIGMA_REL_MIN <= w <= SIGMA_REL_MAX:
            raise ValueError(f"ema_sigma_rel = {text!r}: the width {w} lies outside [{SIGMA_REL_MIN}, {SIGMA_REL_MAX}]")
    if any(b <= a for a, b in zip(widths, widths[1:])):
        raise ValueError(f"ema_sigma_rel = {text!r}: the widths must be strictly increasing")
    return widths


def check_flags(sigma_rel, snapshot_every):
    """-> (widths, snapshot_every) of the two training flags, or a ValueError that names the flag."""
    widths = parse_sigma_rel(sigma_rel)
    try:
        every = int(snapshot_every)
        ok = every >= 0 and every == float(snapshot_every)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"ema_snapshot_every = {snapshot_every!r}: 0 (a snapshot at every save only) or the optimiser steps between snapshots")
    if every > 0 and not widths:
        raise ValueError(f"ema_snapshot_every = {every} without ema_sigma_rel: there is no power-function average to snapshot")
    return widths, every


# ---- snapshot files -----------------------------------------------------------------------------------------------------------------
def layout_digest(n):
    """The 64-bit arena digest (checkpoint.digest_host) of the parameter arena's length n as one little-endian int64: what a snapshot records
    of the layout it belongs to."""
    from . import checkpoint
    return checkpoint.digest_host(np.array([int(n)], dtype="<i8"))


def snapshot_path(logdir, step):
    return Path(logdir) / SNAPSHOT_DIR / f"step_{int(step):09d}.pt"


def write_snapshot(logdir, step, sigma_rel, gamma, arenas):
    """`<logdir>/ema_snapshots/step_<t, 9 digits>.pt`: step, sigma_rel, gamma, the arenas (fp32 [K][n], moved to the host) and the layout
    digest of n.  Written under a temporary name and moved into place, as the checkpoints are.  -> the path"""
    import torch
    arenas = arenas.detach().to("cpu", torch.float32).contiguous()
    assert arenas.dim() == 2 and arenas.shape[0] == len(sigma_rel) == len(gamma), (tuple(arenas.shape), sigma_rel, gamma)
    path = snapshot_path(logdir, step)
    path.parent.mkdir(parents=True, exist_ok=True)
    record = {"step": int(step), "sigma_rel": [float(s) for s in sigma_rel], "gamma": [float(g) for g in gamma], "arenas": arenas,
              "layout": layout_digest(arenas.shape[1])}
    tmp = path.parent / f".{path.name}.tmp{os.getpid()}"
    try:
        torch.save(record, tmp)
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()
    return path


def list_snapshots(logdir):
    """-> [(step, path)] of the snapshot files of a run, by step."""
    found = []
    for path in (Path(logdir) / SNAPSHOT_DIR).glob("step_*.pt"):
        m = re.fullmatch(r"step_(\d{9})\.pt", path.name)
        if m:
            found.append((int(m.group(1)), path))
    return sorted(found)


def _matches(width, wanted):
    return any(abs(width - w) <= 1e-9 for w in wanted)


def gather(logdir, sigma_rel, at_step=None, profiles=None, n=None):
    """The host half of `reconstruct`: read the snapshots with step <= at_step (default: the last snapshot's step), keep the widths named in
    `profiles` (default: all), check them and solve.  n: the arena length the caller's model has (default: the first snapshot's).
    -> {"rows": [fp32 [n] CPU tensors], "snapshots": [(gamma_i, t_i)], "x": float64 [K], "at_step", "gamma", "fit_residual"}"""
    import torch
    target = float(sigma_rel)
    files = list_snapshots(logdir)
    if not files:
        raise ValueError(f"{Path(logdir) / SNAPSHOT_DIR} holds no snapshots: train with --ema_sigma_rel (and --ema_snapshot_every)")
    at_step = files[-1][0] if at_step is None else int(at_step)
    files = [(s, p) for s, p in files if s <= at_step]
    if not files:
        raise ValueError(f"no snapshot of {logdir} has step <= at_step = {at_step}")
    wanted = None if profiles is None else tuple(float(w) for w in profiles)
    rows, snaps, widths = [], [], set()
    for step, path in files:
        rec = torch.load(path, map_location="cpu")
        arenas = rec["arenas"]
        n = arenas.shape[1] if n is None else int(n)
        if arenas.shape[1] != n or rec["layout"] != layout_digest(n):
            raise ValueError(f"{path} holds arenas of {arenas.shape[1]} parameters (layout digest {rec['layout']:#018x}), this model has {n} "
                             f"({layout_digest(n):#018x}): the snapshot was written by a model of another shape")
        for k, (width, gamma) in enumerate(zip(rec["sigma_rel"], rec["gamma"])):
            if wanted is None or _matches(width, wanted):
                rows.append(arenas[k])
                snaps.append((float(gamma), int(rec["step"])))
                widths.add(float(width))
    if not rows:
        raise ValueError(f"profiles = {profiles}: none of the snapshots of {logdir} tracks one of these widths")
    lo, hi = min(widths) / RANGE_FACTOR, max(widths) * RANGE_FACTOR
    if not lo <= target <= hi or not 0.0 < target < SIGMA_REL_SUP:
        raise ValueError(f"sigma_rel = {target}: the snapshots track the widths {sorted(widths)}, which reach [{lo:.4g}, {hi:.4g}] (the tracked "
                         f"range widened by {RANGE_FACTOR} on each side)")
    if len(rows) > MAX_ARENAS:
        raise ValueError(f"{len(rows)} arenas with step <= {at_step}: one reconstruction combines at most {MAX_ARENAS} - give an earlier "
                         f"at_step, fewer profiles, or thin the snapshots with a stride")
    gamma = gamma_from_sigma_rel(target)
    x = solve_weights(snaps, gamma, at_step)
    return {"rows": rows, "snapshots": snaps, "x": x, "at_step": at_step, "gamma": gamma, "fit_residual": fit_residual(snaps, gamma, at_step, x)}


# ---- the device half ----------------------------------------------------------------------------------------------------------------
def combine(found, device="cuda"):
    """sum_i x_i row_i of gather()'s result on the device (ops.arena_combine).  -> fp32 [n]"""
    import torch

    from . import ops
    rows = found["rows"]
    n = rows[0].numel()
    stack = torch.zeros((len(rows), (n + 3) // 4 * 4), dtype=torch.float32, device=device)      # a row stride that keeps 16-byte loads
    for k, row in enumerate(rows):
        stack[k, :n].copy_(row)
    return ops.arena_combine(stack, found["x"], n=n)


def reconstruct(logdir, sigma_rel, at_step=None, profiles=None, device="cuda", n=None):
    """The power-function average of relative width `sigma_rel` at step `at_step` (default: the last snapshot's step - a target past it is
    fitted much worse) as a combination of the run's snapshots, optionally of the tracked widths in `profiles` alone.  -> device fp32 [n]"""
    return combine(gather(logdir, sigma_rel, at_step=at_step, profiles=profiles, n=n), device)


def install(model, arena):
    """Write an arena into the model's net (and into its weight average, which sample() and the likelihoods run, when ema_decay is on)."""
    nets = [model.net] + ([model.ema_net] if getattr(model, "ema_net", None) is not None else [])
    for net in nets:
        net.flat_params.copy_(arena)
        net.mark_params_changed()
    if len(nets) > 1:
        model.optimizer.ema_seeded = True


def _float_list(text):
    return tuple(float(p) for p in text.split(",") if p.strip())


def sweep(model, batches, logdir, widths, at_step=None, profiles=None):
    """model.loss on `batches` under the reconstruction of every width and under the online weights, the model's Philox counters put back
    between candidates.  -> (columns, rows) as written to <logdir>/ema_sweep.csv"""
    import torch
    online = model.net.flat_params.clone()
    n = online.numel()
    streams = (model.diffusion.rng.state_dict(), model._aux_rng.state_dict(), model.net.dropout_state())
    rows, keys = [], []
    model.eval()
    for width in tuple(widths) + (None,):
        if width is None:
            arena, head = online, {"sigma_rel": "online", "at_step": "", "n_arenas": "", "fit_residual": ""}
        else:
            found = gather(logdir, width, at_step=at_step, profiles=profiles, n=n)
            arena = combine(found, online.device)
            head = {"sigma_rel": f"{width:.9g}", "at_step": found["at_step"], "n_arenas": len(found["rows"]),
                    "fit_residual": f"{found['fit_residual']:.6e}"}
        install(model, arena)
        model.diffusion.rng.load_state_dict(streams[0])
        model._aux_rng.load_state_dict(streams[1])
        model.net.load_dropout_state(streams[2])
        sums = {}
        with torch.no_grad():
            for x, y in batches:
                for key, val in model.loss(x, y.clone())[1].items():
                    sums[key] = sums.get(key, 0.0) + float(val)
        for key in sums:
            if key not in keys:
                keys.append(key)
            head[key] = f"{sums[key] / len(batches):.9g}"
        rows.append(head)
    install(model, online)
    columns = ["sigma_rel", "at_step", "n_arenas", "fit_residual"] + [k for k in keys if k != "nlogp"] + (["nlogp"] if "nlogp" in keys else [])
    with open(Path(logdir) / SWEEP_FILE, "w", newline="") as f:
        writer = csv.DictWriter(f, fieldnames=columns, restval="")
        writer.writeheader()
        writer.writerows(rows)
    return columns, rows


def main(argv=None):
    import torch

    from . import main as driver
    ap = argparse.ArgumentParser(description="reconstruct the weights of an EMA width from a run's power-function snapshots")
    ap.add_argument("--run", type=Path, required=True, help="the run's logdir (hps.yaml, model.pt, ema_snapshots/)")
    ap.add_argument("--sigma_rel", type=float, required=True)
    ap.add_argument("--at_step", type=int, default=None)
    ap.add_argument("--profiles", type=_float_list, default=None, help="use only these tracked widths, e.g. 0.05,0.1")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--sweep", type=_float_list, default=())
    ap.add_argument("--sweep_batches", type=int, default=4)
    ap.add_argument("--nlogp_samples", type=int, default=0)
    args = ap.parse_args(argv)
    if args.sweep and args.sweep_batches < 1:
        raise ValueError(f"--sweep_batches {args.sweep_batches}: at least one test batch")
    flags = ["--weights_from", str(args.run / "model.pt"), "--eval_heavy", "0"]
    if args.nlogp_samples > 0:
        flags += ["--nlogp_samples", str(args.nlogp_samples)]
    model, _, test_ds, _, _, G = driver.load_model_and_data(flags)
    device = model.net.flat_params.device
    n = model.net.flat_params.numel()
    found = gather(args.run, args.sigma_rel, at_step=args.at_step, profiles=args.profiles, n=n)
    print(f"sigma_rel {args.sigma_rel:g} at step {found['at_step']}: {len(found['rows'])} arenas, fit residual {found['fit_residual']:.3e}, "
          f"sum of coefficients {float(found['x'].sum()):.6f}")
    if args.sweep:
        batches = [(x.to(device), y.to(device)) for x, y in itertools.islice(iter(test_ds), args.sweep_batches)]
        columns, rows = sweep(model, batches, args.run, args.sweep, at_step=args.at_step, profiles=args.profiles)
        print("\n".join(",".join(str(r.get(c, "")) for c in columns) for r in [dict(zip(columns, columns))] + rows))
    model.net.flat_params.copy_(combine(found, device))
    model.net.mark_params_changed()
    out = args.out if args.out is not None else args.run / f"model_ema_{args.sigma_rel:g}.pt"
    torch.save({"net." + k: v.detach().cpu() for k, v in model.net.state_dict().items()}, out)
    print("WROTE", out)
    return out


if __name__ == "__main__":
    main()
