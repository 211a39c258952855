"""GPU tests of metrics.manifold_metrics on the HIP kernels and of the driver end to end: an autoencoder trained here feeds the heavy
evaluation of a diffusion run, at the reference's 500-sample path and at --eval_heavy_samples."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _integer_rows(n, D, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(n, D)).astype(np.float32)


@pytest.mark.parametrize("M,Q,D", [(64, 50, 64), (37, 41, 5), (40, 40, 256), (1100, 300, 64)])
def test_manifold_metrics_on_the_device_equal_the_cpu_path(M, Q, D):
    from generative_models_amd import metrics
    real, gen = torch.from_numpy(_integer_rows(M, D, 1)), torch.from_numpy(_integer_rows(Q, D, 2))
    on_cpu = metrics.manifold_metrics(real, gen, k=3)
    on_gpu = metrics.manifold_metrics(real.cuda(), gen.cuda(), k=3)
    want = knn_ref.manifold(real.numpy(), gen.numpy(), 3)
    for key in ("precision", "recall", "density", "coverage"):
        assert on_gpu[key].is_cuda and float(on_gpu[key]) == float(on_cpu[key]) == np.float32(want[key]), key
    # f1 = 2 p r / (p + r) from equal p and r: four fp32 roundings on either device, 2^-24 each
    assert np.isclose(float(on_gpu["f1"]), float(on_cpu["f1"]), rtol=4 * 2.0 ** -24, atol=0.0, equal_nan=True)
    # The Fréchet distance from device moments against compute_fid on the host.  Both take the Z eigenvalues of S_a S_b in float64; each
    # carries an absolute error of the order of 2^-52 |S_a| |S_b|, and where the product is rank-deficient (fewer rows than Z + 1) the
    # square root of a zero eigenvalue turns that into sqrt(2^-52 |S_a| |S_b|): Z of those is the bound.
    scores = metrics.score_latents(real.cuda(), gen.cuda(), 3)
    norms = [np.linalg.norm(np.cov(t.numpy().astype(np.float64), rowvar=False), 2) for t in (real, gen)]
    bound = D * np.sqrt(2.0 ** -52 * norms[0] * norms[1])
    want_fid = metrics.compute_fid(gen.numpy(), real.numpy())
    print("fid", scores["fid"], want_fid, "bound", bound)
    assert abs(scores["fid"] - want_fid) <= bound


def _run(*flags):
    """One run of the driver in this process (a child process spends most of its seconds importing torch) -> the keys and means of its final
    evaluation pass, as dump_logger prints them."""
    from generative_models_amd import main
    final = main.train(*main.load_model_and_data(list(flags)))
    return {key: float(np.mean(val)) for key, val in final.items()}


def test_a_trained_autoencoder_feeds_the_heavy_evaluation(tmp_path):
    import yaml
    arbiter, plain, scaled = tmp_path / "autoencoder", tmp_path / "plain", tmp_path / "scaled"
    trained = _run("--model=autoencoder", "--epochs", "1", "--hidden_size", "16", "--bs", "64", "--train_batches", "8", "--test_batches", "1",
                   "--save_n", "1", "--logdir", str(arbiter))          # save_n 1: the file of the last checkpoint holds the trained weights
    print("autoencoder run", trained)
    assert np.isfinite(trained["autoencoder/train/recon_loss"]) and (arbiter / "model.jit.pt").exists()
    diffusion = ("--model=diffusion", "--hidden_size", "32", "--timesteps", "4", "--bs", "64", "--epochs", "0", "--eval_heavy", "1", "--autoencoder",
                 str(arbiter / "model.jit.pt"))
    old_keys = {"eval/" + cond + key for cond in ("", "cond_") for key in ("fid", "precision", "recall", "f1")} | {"eval/centroid_classifier_loss"}
    new_keys = {"eval/" + cond + key for cond in ("", "cond_") for key in ("density", "coverage")} | {"eval/heavy_samples"}
    new_keys |= {"dt/eval_heavy_" + key for key in ("sampling", "embedding", "metrics")}
    before = set(_run(*diffusion, "--logdir", str(plain)))
    assert {key for key in before if key.startswith("eval/")} == old_keys and not (new_keys & before)          # exactly the old eval/* keys
    logged = _run(*diffusion, "--eval_heavy_samples", "128", "--logdir", str(scaled))
    assert set(logged) == before | new_keys                                            # today's keys, and the new ones only with the flag
    for key in ("eval/fid", "eval/precision", "eval/recall", "eval/density", "eval/coverage"):
        assert np.isfinite(logged[key]), (key, logged[key])
    assert logged["eval/heavy_samples"] >= 128
    hps = yaml.load((scaled / "hps.yaml").read_text(), Loader=yaml.Loader)
    assert hps["eval_heavy_samples"] == 128 and hps["arbiters"] == "stand-in"          # the classifier of this run is the centroid stand-in
