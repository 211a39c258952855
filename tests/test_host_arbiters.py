"""Host tests of the trainable arbiters (generative_models_amd/arbiter_models.py) against vectors of the reference's own classes
(tests/golden/arbiters_s28.npz, tools/make_arbiter_golden.py), of their save() / --autoencoder round trip through the driver, and of
metrics.manifold_metrics' CPU path against the float64 restatement tests/knn_ref.py."""
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Golden comparison: the bar set for it is 1e-5 (the larger of rtol and atol).  Measured on the CPU: encoder output, logits, full_loss,
# recon_loss, z_mean and z_std equal the golden bit for bit; kl_loss differs by 2.3e-10 absolute = 1.0e-7 relative (0.5 z^2 here against
# torch.distributions' kl_divergence there).  Far below the bar, so the tolerance is ten times the measured value.
TOL = 1e-6


def _flags(Model, **over):
    from generative_models_amd import common
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=16, lr=3e-4, bs=64, pad32=0, model=Model.__name__.lower(), device="cpu")
    G.update(over)
    return G


def _models():
    from generative_models_amd import arbiter_models
    return arbiter_models.Autoencoder, arbiter_models.Classifier


def _golden_state(g, prefix):
    return {key[len(prefix):]: torch.from_numpy(g[key]) for key in g.files if key.startswith(prefix) and "/metric/" not in key}


def _close(got, want):
    return np.allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=TOL, atol=TOL)


@pytest.mark.parametrize("binarize", [0, 1])
def test_autoencoder_matches_the_reference_classes(golden, binarize):
    Autoencoder, _ = _models()
    g = golden("arbiters_s28.npz")
    model = Autoencoder(_flags(Autoencoder, binarize=binarize))
    want = _golden_state(g, f"ae_b{binarize}/")
    have = model.state_dict()
    assert list(have) == list(want) and all(have[key].shape == want[key].shape for key in want)          # the reference's keys, in its order
    model.load_state_dict(want)
    x = torch.from_numpy(g[f"x_b{binarize}"])
    with torch.no_grad():
        z = model(x)
        _, metrics = model.loss(x)
    assert tuple(z.shape) == (8, 64) and _close(z.numpy(), g[f"z_b{binarize}"])
    assert set(metrics) == {"full_loss", "recon_loss", "kl_loss", "z_mean", "z_std"}
    for key, val in metrics.items():
        print(key, float(val), float(g[f"ae_b{binarize}/metric/{key}"]))
        assert _close(float(val), float(g[f"ae_b{binarize}/metric/{key}"])), key


def test_classifier_matches_the_reference_class(golden):
    _, Classifier = _models()
    g = golden("arbiters_s28.npz")
    model = Classifier(_flags(Classifier))
    want = _golden_state(g, "clf/")
    have = model.state_dict()
    assert list(have) == list(want) and all(have[key].shape == want[key].shape for key in want)
    assert Classifier.DG.epochs == 6 and Classifier.DG.save_n == 1
    model.load_state_dict(want)
    x, y = torch.from_numpy(g["x_b0"]), torch.from_numpy(g["y"])
    with torch.no_grad():
        logits = model(x)
        _, metrics = model.loss(x, y)
    assert tuple(logits.shape) == (8, 10) and _close(logits.numpy(), g["logits"])
    assert set(metrics) == {"cross_entropy_loss"} and _close(float(metrics["cross_entropy_loss"]), float(g["clf/metric/cross_entropy_loss"]))


@pytest.mark.parametrize("C,S", [(3, 32), (1, 64)])
def test_other_sizes(C, S):
    Autoencoder, Classifier = _models()
    model = Autoencoder(_flags(Autoencoder, in_channels=C, image_size=S))
    x = torch.rand(3, C, S, S) * 2 - 1
    with torch.no_grad():
        z = model(x)
        assert tuple(z.shape) == (3, 64) and tuple(model.decoder(z).shape) == (3, C, S, S)
        assert tuple(Classifier(_flags(Classifier, in_channels=C, image_size=S))(x).shape) == (3, 10)
        assert np.isfinite(float(model.loss(x)[0]))
        with pytest.raises(ValueError):
            model.loss(x[:, :, :28, :28])


@pytest.mark.parametrize("S", [30, 20])
def test_sizes_the_decoder_cannot_emit_raise(S):
    for Model in _models():
        with pytest.raises(ValueError):
            Model(_flags(Model, image_size=S))


def test_thirty_adam_steps_lower_both_losses():
    """30 steps on one batch of the synthetic source.  Its labels are drawn independently of its images, so a classifier can only fit the
    batch it sees: both losses are read on the batch that is trained on.  Reductions of this run, measured: recon_loss 1.5494 -> 1.4457
    (0.1037), cross_entropy_loss 2.3032 -> 2.2610 (0.0421); half of each is asserted."""
    from generative_models_amd import data
    for Model, key, least in zip(_models(), ("recon_loss", "cross_entropy_loss"), (0.052, 0.021)):
        torch.manual_seed(20260)
        model = Model(_flags(Model))
        batch = next(iter(data.SyntheticMNIST(64, 1, 0, 0, "cpu", seed=2000)))
        with torch.no_grad():
            before = float(model.loss(*batch)[1][key])
        for _ in range(30):
            model.train_step(*batch)
        with torch.no_grad():
            after = float(model.loss(*batch)[1][key])
        print(key, before, after)
        assert before - after >= least, (key, before, after)


class _NoiseModel:
    """What eval_heavy asks of a model: sample(n, y)."""

    def sample(self, n, y=None):
        return torch.rand(n, 1, 28, 28) * 2 - 1


def test_save_round_trip_and_the_key_space(tmp_path):
    from generative_models_amd import common, data, main, metrics
    Autoencoder, Classifier = _models()
    for Model in (Autoencoder, Classifier):
        model = Model(_flags(Model))
        out = tmp_path / Model.__name__
        out.mkdir()
        model.save(out, torch.rand(4, 1, 28, 28) * 2 - 1)
        assert (out / "model.pt").exists() and (out / "model.jit.pt").exists()
        loaded = torch.jit.load(str(out / "model.jit.pt"))
        x = torch.rand(7, 1, 28, 28) * 2 - 1                                  # another batch size than the trace saw
        with torch.no_grad():
            assert torch.equal(loaded(x), model(x))
        assert set(torch.load(out / "model.pt")) == set(model.state_dict())
    G = common.AttrDict(eval_heavy=1, class_cond=0, autoencoder=tmp_path / "Autoencoder" / "model.jit.pt", classifier=tmp_path / "none.pt",
                        device="cpu", bs=16)
    autoencoder, classifier = main._feature_extractors(G, "cpu")
    assert classifier is None and not getattr(autoencoder, "stand_in", False) and G.arbiters == "reference"          # no hps.yaml beside it
    (tmp_path / "Autoencoder" / "hps.yaml").write_text("model: autoencoder\n")
    main._feature_extractors(G, "cpu")
    assert G.arbiters == "trained"
    logger = defaultdict(list)
    metrics.eval_heavy(logger, _NoiseModel(), data.SyntheticMNIST(16, 2, 0, 0, "cpu", seed=5), autoencoder, None, G, total_samples=32)
    assert set(logger) == {"eval/fid", "eval/precision", "eval/recall", "eval/f1"} and np.isfinite(logger["eval/fid"][0])
    G.eval_heavy_samples, G.eval_heavy_k = 40, 3
    logger = defaultdict(list)
    metrics.eval_heavy(logger, _NoiseModel(), data.SyntheticMNIST(16, 2, 0, 0, "cpu", seed=5), autoencoder, None, G)
    assert {"eval/fid", "eval/precision", "eval/recall", "eval/f1", "eval/density", "eval/coverage", "eval/heavy_samples"} <= set(logger)
    assert not any("randfeat" in key for key in logger) and logger["eval/heavy_samples"][0] == 48 and np.isfinite(logger["eval/fid"][0])
    G.autoencoder = tmp_path / "none.pt"
    stand_in, _ = main._feature_extractors(G, "cpu")
    assert stand_in.stand_in and G.arbiters == "stand-in"


def test_cli_trains_an_autoencoder_on_the_cpu(tmp_path):
    cmd = [sys.executable, "-m", "generative_models_amd.main", "--model=autoencoder", "--device", "cpu", "--epochs", "1", "--hidden_size", "16",
           "--train_batches", "4", "--test_batches", "1", "--save_images", "1", "--logdir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("model.pt", "model.jit.pt", "hps.yaml", os.path.join("images", "reconstruction_0000.png")):
        assert (tmp_path / name).exists(), name
    assert "autoencoder/train/recon_loss" in r.stdout and "autoencoder/test/z_std" in r.stdout
    from generative_models_amd import main
    assert main._trained_here(tmp_path / "model.jit.pt") and not main._trained_here(tmp_path / "images" / "model.jit.pt")
    z = torch.jit.load(str(tmp_path / "model.jit.pt"))(torch.zeros(3, 1, 28, 28))
    assert tuple(z.shape) == (3, 64)


def _integer_rows(n, D, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(n, D)).astype(np.float32)


@pytest.mark.parametrize("M,Q,D", [(64, 50, 64), (37, 41, 5), (40, 40, 256)])
def test_manifold_metrics_on_the_cpu_equal_the_float64_restatement(M, Q, D):
    """Integer-valued features in [-4, 4]: every d2 is an integer of at most 64 D <= 16,384, exact in fp32 in any summation order."""
    from generative_models_amd import metrics
    real, gen = _integer_rows(M, D, 1), _integer_rows(Q, D, 2)
    got = metrics.manifold_metrics(torch.from_numpy(real), torch.from_numpy(gen), k=3)
    want = knn_ref.manifold(real, gen, 3)
    assert set(got) == set(want) == {"precision", "recall", "f1", "density", "coverage"}
    for key in ("precision", "recall", "density", "coverage"):
        assert float(got[key]) == np.float32(want[key]), (key, float(got[key]), want[key])
    assert np.isclose(float(got["f1"]), want["f1"], rtol=1e-6, equal_nan=True)
    r2 = metrics._radius2(torch.from_numpy(real), 3)
    assert np.array_equal(r2.numpy().astype(np.float64), knn_ref.radius2(real, 3))
    q_count, m_count = metrics._ball_counts(torch.from_numpy(real), r2, torch.from_numpy(gen))
    want_q, want_m = knn_ref.counts(real, r2.numpy(), gen)
    assert np.array_equal(q_count.numpy(), want_q) and np.array_equal(m_count.numpy(), want_m)
    if len(np.unique(real, axis=0)) == M:                                       # no two rows coincide: every ball holds its own centre
        same = metrics.manifold_metrics(torch.from_numpy(real), torch.from_numpy(real), k=3)
        assert float(same["precision"]) == float(same["recall"]) == float(same["coverage"]) == 1.0


def test_heavy_eval_scores_a_sample_file(tmp_path, capsys):
    import json
    from generative_models_amd import heavy_eval, metrics
    Autoencoder, _ = _models()
    model = Autoencoder(_flags(Autoencoder))
    model.save(tmp_path)
    rng = np.random.default_rng(3)
    real, samples = rng.integers(0, 256, size=(90, 28, 28), dtype=np.uint8), rng.integers(0, 256, size=(70, 1, 28, 28), dtype=np.uint8)
    for split in ("train", "test"):
        np.save(tmp_path / f"{split}_images.npy", real)
        np.save(tmp_path / f"{split}_labels.npy", np.zeros(90, dtype=np.uint8))
    np.save(tmp_path / "samples_images.npy", samples)
    scores = heavy_eval.main(["--samples", str(tmp_path / "samples_images.npy"), "--data", "npy", "--data_root", str(tmp_path), "--autoencoder",
                              str(tmp_path / "model.jit.pt"), "--device", "cpu", "--bs", "32"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == scores
    with torch.no_grad():
        z_real = model(torch.from_numpy(real)[:, None].float() / 255 * 2 - 1)
        z_gen = model(torch.from_numpy(samples).float() / 255 * 2 - 1)
    want = metrics.manifold_metrics(z_real, z_gen, 3)
    assert scores["samples"] == 70 and scores["real"] == 90 and scores["encoder"] == "reference"
    # one batch here, batches of 32 there: the convolutions may round differently, the counts only move if a pair sits on a ball's edge
    for key in ("precision", "recall", "density", "coverage"):
        assert abs(scores[key] - float(want[key])) <= 2 / 70, key
    assert np.isclose(scores["fid"], metrics.compute_fid(z_gen.numpy(), z_real.numpy()), rtol=1e-3, atol=1e-9)
