"""Sample-quality metrics of the heavy evaluation, written from their definitions:

* Fréchet distance between two Gaussians fitted to latent sets — the quantity the reference logs as `eval/fid`
  (gms/common.py:267-288).  d = m(mu_a, mu_b) + tr(S_a) + tr(S_b) - 2 tr((S_a S_b)^(1/2)), with the reference's one deviation
  from the textbook formula kept: m is the MEAN of the squared mean differences, not their sum.
* k-NN manifold precision / recall / F1 (Kynkäänniemi et al., arXiv 1904.06991; gms/common.py:291-319): a point is covered by a
  set if it lies strictly inside the k-th-neighbour ball of at least one member of the set.
* `eval_heavy`: the sampling loop of gms/main.py:95-149 that feeds them (same metric keys, `y = -1` = unconditional).

* `manifold_metrics` / `eval_heavy_at_scale` (an extension, `--eval_heavy_samples N`): the same quantities plus density and coverage
  (Naeem et al., arXiv 2002.09797) at sample counts where two N x N distance matrices no longer fit - k-NN radii and ball counts from two
  HIP kernels that never form the matrix (csrc/knn_f32.hip), the Fréchet distance from float64 moments taken on the device.

Everything here works on [N, Z] latents of a feature extractor passed in by the caller (a TorchScript autoencoder / classifier trained with
arbiter_models.py or brought from elsewhere, or the stand-ins of arbiters.py).  Off the throughput path."""
import numpy as np
import torch
import torch.nn.functional as F


def _trace_sqrt_product(cov_a, cov_b):
    """tr((A B)^(1/2)) for covariance matrices: the principal square root has the square roots of the eigenvalues of A B as
    its eigenvalues, so its trace is their sum (complex arithmetic: round-off can push a zero eigenvalue below zero)."""
    eig = np.linalg.eigvals(cov_a @ cov_b).astype(np.complex128)
    return np.sqrt(eig).sum()


def compute_fid(x, y):
    """x, y: [N, Z] numpy latents -> float; NaN for anything that cannot be evaluated (wrong rank, too few rows, a failed
    eigen-decomposition) — the reference swallows every failure into NaN too."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1] or min(x.shape[0], y.shape[0]) < 2:
        return np.nan
    try:
        mean_term = np.mean(np.square(x.mean(axis=0) - y.mean(axis=0)))
        cov_x = np.atleast_2d(np.cov(x, rowvar=False))
        cov_y = np.atleast_2d(np.cov(y, rowvar=False))
        value = mean_term + np.trace(cov_x) + np.trace(cov_y) - 2.0 * _trace_sqrt_product(cov_x, cov_y)
        return float(np.real(value))
    except (np.linalg.LinAlgError, ValueError, FloatingPointError):
        return np.nan


def knn_radii(points, k):
    """Distance from every point to its k-th nearest OTHER point of the same set ([N] tensor)."""
    pairwise = torch.cdist(points, points)
    return pairwise.kthvalue(k + 1, dim=1).values            # position 0 of the sorted row is the point itself (distance 0)


def coverage(manifold, queries, k=3):
    """Fraction of `queries` lying strictly inside at least one k-NN ball of `manifold`."""
    inside = torch.cdist(queries, manifold) < knn_radii(manifold, k)[None, :]
    return inside.any(dim=1).float().mean()


def precision_recall_f1(*, real, gen, k=3):
    precision = coverage(real, gen, k)            # generated samples that fall on the data manifold
    recall = coverage(gen, real, k)               # data points the generated manifold reaches
    return {"precision": precision, "recall": recall, "f1": 2 * (precision * recall) / (precision + recall)}


CPU_PAIR_BUDGET = 1 << 24          # floats of (a - b) one chunk of the CPU path may hold


def _cpu_d2(a, b):
    """[A, B] fp32: sum_i (a[i] - b[i])^2 of every pair, the direct difference (the kernels' definition; here torch's summation order)."""
    return (a[:, None, :] - b[None, :, :]).square().sum(-1)


def _cpu_chunks(rows, cols, D):
    step = max(1, CPU_PAIR_BUDGET // max(1, cols * D))
    return range(0, rows, step), step


def _radius2(points, k):
    """[N] fp32: the (k + 1)-th smallest squared distance of every point to the points of its set, itself (0) included."""
    if points.is_cuda:
        from . import ops
        return ops.knn_radius2(points, k)
    N, D = points.shape
    if not 1 <= k < N:
        raise ValueError(f"k = {k} with {N} points (1 .. N - 1)")
    out = torch.empty((N,), dtype=torch.float32)
    starts, step = _cpu_chunks(N, N, D)
    for lo in starts:
        out[lo:lo + step] = _cpu_d2(points[lo:lo + step], points).kthvalue(k + 1, dim=1).values
    return out


def _ball_counts(balls, r2, queries):
    """(q_count [Q], m_count [M]) int32: how many balls hold each query, how many queries each ball holds; d2 < r2, strict."""
    if balls.is_cuda:
        from . import ops
        return ops.ball_counts(balls, r2, queries)
    (M, D), Q = balls.shape, queries.shape[0]
    q_count, m_count = torch.empty((Q,), dtype=torch.int32), torch.zeros((M,), dtype=torch.int32)
    starts, step = _cpu_chunks(Q, M, D)
    for lo in starts:
        inside = _cpu_d2(queries[lo:lo + step], balls) < r2[None, :]
        q_count[lo:lo + step] = inside.sum(1)
        m_count += inside.sum(0)
    return q_count, m_count


def manifold_metrics(real, gen, k=3):
    """precision / recall / f1 as precision_recall_f1 defines them, plus density and coverage (Naeem et al., arXiv 2002.09797), without a
    distance matrix: real [M, Z], gen [Q, Z] fp32 on one device -> dict of 0-d tensors.
      precision = mean(q_count > 0), density = sum(q_count) / (k Q), coverage = mean(m_count > 0)   for the real set's k-NN balls and the
                  generated queries (one count launch),
      recall    = mean(q_count > 0)                                                                   with the roles swapped.
    CUDA tensors: ops.knn_radius2 / ops.ball_counts (two launches each, csrc/knn_f32.hip); CPU tensors: the same definition in chunked torch.
    Squared distances against squared radii: the comparison precision_recall_f1 makes after two square roots."""
    real, gen = real.float().contiguous(), gen.float().contiguous()
    if real.dim() != 2 or gen.dim() != 2 or real.shape[1] != gen.shape[1] or real.device != gen.device:
        raise ValueError(f"manifold_metrics: real {tuple(real.shape)} on {real.device}, gen {tuple(gen.shape)} on {gen.device}")
    q_gen, m_real = _ball_counts(real, _radius2(real, k), gen)
    q_real, _ = _ball_counts(gen, _radius2(gen, k), real)
    share = lambda hit: hit.sum().double().div(hit.numel()).float()          # in float64, then rounded once: the same fp32 on either device
    precision, recall = share(q_gen > 0), share(q_real > 0)
    return {"precision": precision, "recall": recall, "f1": 2 * (precision * recall) / (precision + recall),
            "density": q_gen.sum().double().div(k * gen.shape[0]).float(), "coverage": share(m_real > 0)}


def latent_moments(z):
    """(mean [Z], covariance [Z, Z]) of latents [N, Z] in float64 on their device: np.mean / np.cov(rowvar=False) (N - 1 in the denominator)."""
    z = z.double()
    mean = z.mean(0)
    centred = z - mean
    return mean, centred.t() @ centred / (z.shape[0] - 1)


def fid_from_moments(mean_a, cov_a, mean_b, cov_b):
    """compute_fid's formula on moments taken elsewhere (the latents stay on the device; 2 (Z + Z^2) doubles come to the host)."""
    mean_a, cov_a, mean_b, cov_b = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (mean_a, cov_a, mean_b, cov_b))
    try:
        value = np.mean(np.square(mean_a - mean_b)) + np.trace(cov_a) + np.trace(cov_b) - 2.0 * _trace_sqrt_product(cov_a, cov_b)
        return float(np.real(value))
    except (np.linalg.LinAlgError, ValueError, FloatingPointError):
        return np.nan


class _LatentBank:
    """Named lists of latent batches, concatenated on demand."""

    def __init__(self):
        self._rows = {}

    def add(self, name, z):
        self._rows.setdefault(name, []).append(z.detach().float())

    def get(self, name):
        return torch.cat(self._rows[name])


@torch.inference_mode()
def eval_heavy(logger, model, test_ds, autoencoder, classifier, G, total_samples=500):
    """Draw at least `total_samples` samples batch by batch (unconditional: y = -1; additionally class-conditional when
    G.class_cond), embed samples and test images, log eval/fid, eval/precision|recall|f1 (+ cond_* and classifier_loss).
    The reference also logs ignite's own FID (`ignite_fid`); pytorch-ignite is not installed here, so that key is absent.
    G.eval_heavy_samples = N > 0 hands over to eval_heavy_at_scale."""
    if int(G.get("eval_heavy_samples", 0)) > 0:
        return eval_heavy_at_scale(logger, model, test_ds, autoencoder, classifier, G, int(G.eval_heavy_samples), int(G.get("eval_heavy_k", 3)))
    bank = _LatentBank()
    clf_losses = []
    drawn = 0
    for x, y in ((b[0].to(G.device), b[1].to(G.device)) for b in test_ds):
        n = x.shape[0]
        if G.class_cond:
            guided = model.sample(n, y=y)
            clf_losses.append(F.cross_entropy(classifier(guided), y).item())
            bank.add("cond", autoencoder(guided))
        bank.add("gen", autoencoder(model.sample(n, y=torch.full_like(y, -1))))
        bank.add("real", autoencoder(x))
        drawn += n
        if drawn >= total_samples:
            break
    real = bank.get("real")

    def against_real(name):
        gen = bank.get(name)
        scores = precision_recall_f1(real=real, gen=gen)
        scores["fid"] = compute_fid(gen.cpu().numpy(), real.cpu().numpy())
        return scores

    # The reference's metric keys (`eval/fid`, `eval/precision` ...) are kept for values taken in the REFERENCE's feature space (its
    # TorchScript arbiters).  With the stand-ins of arbiters.py the same quantities are logged as `eval/randfeat_*` /
    # `eval/centroid_classifier_loss`, so that a log or hps file can never pass them off as reference-space numbers.
    space = "randfeat_" if getattr(autoencoder, "stand_in", False) else ""
    results = {space + key: val for key, val in against_real("gen").items()}
    if G.class_cond:
        results[("centroid_" if getattr(classifier, "stand_in", False) else "") + "classifier_loss"] = clf_losses
        results.update({space + "cond_" + key: val for key, val in against_real("cond").items()})
    for key, val in results.items():
        val = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else val
        logger[f"eval/{key}"] += [float(np.mean(val))]
    return results


def _now(device):
    import time
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return time.time()


def score_latents(real, gen, k=3):
    """-> {fid, precision, recall, f1, density, coverage} as floats for latents [M, Z] / [Q, Z] on one device: the Fréchet distance from float64
    moments (compute_fid's formula) and manifold_metrics.  What eval_heavy_at_scale and heavy_eval.py log."""
    scores = {key: float(val) for key, val in manifold_metrics(real, gen, k).items()}
    scores["fid"] = fid_from_moments(*latent_moments(gen), *latent_moments(real)) if min(real.shape[0], gen.shape[0]) >= 2 else float("nan")
    return scores


@torch.inference_mode()
def eval_heavy_at_scale(logger, model, test_ds, autoencoder, classifier, G, samples, k=3):
    """The heavy evaluation at `samples` >= 1 samples (--eval_heavy_samples; the reference stops at 500): at least `samples` unconditional
    samples in batches of G.bs (with G.class_cond as many guided ones, labels arange % 10, scored by the classifier), the first
    min(samples, test-set size) test images of THIS rank's shard; the latents stay on the device, score_latents does the rest.  Logs
    eval_heavy's keys plus eval/density, eval/coverage, eval/heavy_samples (+ the cond_ forms) and where the time went
    (dt/eval_heavy_sampling | embedding | metrics).  One rank's samples only: nothing is gathered across ranks."""
    bs = int(G.bs)
    device = getattr(model, "run_device", G.device)
    took = {"sampling": 0.0, "embedding": 0.0, "metrics": 0.0}
    bank = _LatentBank()
    clf_losses = []

    def embed(name, x):
        started = _now(x.device)
        bank.add(name, autoencoder(x))
        took["embedding"] += _now(x.device) - started

    seen = 0
    for x, y in ((b[0].to(device), b[1].to(device)) for b in test_ds):
        x = x[:samples - seen]
        embed("real", x)
        seen += x.shape[0]
        if seen >= samples:
            break
    if seen == 0:
        raise ValueError("eval_heavy_at_scale: the test loader yielded no batch (fewer test images than --bs on this rank?): nothing to compare "
                         "the samples with")
    drawn = 0
    while drawn < samples:
        started = _now(device)
        y = (torch.arange(drawn, drawn + bs, device=device) % 10).long()
        free = model.sample(bs, y=torch.full_like(y, -1))
        guided = model.sample(bs, y=y) if G.class_cond else None
        took["sampling"] += _now(device) - started
        embed("gen", free)
        if guided is not None:
            clf_losses.append(F.cross_entropy(classifier(guided), y).item())
            embed("cond", guided)
        drawn += bs
    real = bank.get("real")
    started = _now(device)
    space = "randfeat_" if getattr(autoencoder, "stand_in", False) else ""
    results = {space + key: val for key, val in score_latents(real, bank.get("gen"), k).items()}
    results["heavy_samples"] = drawn
    if G.class_cond:
        results[("centroid_" if getattr(classifier, "stand_in", False) else "") + "classifier_loss"] = clf_losses
        results.update({space + "cond_" + key: val for key, val in score_latents(real, bank.get("cond"), k).items()})
    took["metrics"] = _now(device) - started
    for key, val in results.items():
        logger[f"eval/{key}"] += [float(np.mean(val))]
    for key, val in took.items():
        logger[f"dt/eval_heavy_{key}"] += [val]
    return results
