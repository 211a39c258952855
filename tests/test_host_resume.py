"""CPU tests (no GPU) of resumable training: the arena digest against its pure-Python restatement and known answers, the C ABI entry and its
argument checks, the state round trips of the streams, loaders and optimiser, the --save_state / --resume flags and every error path of a
resume that needs no GPU."""
import ctypes
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_ref  # noqa: E402


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=32)
    G.update(flags)
    return Model(G)


# ---- the digest ----------------------------------------------------------------------------------------------------------------------
def test_reference_known_answers():
    for words, want in digest_ref.KNOWN:
        assert digest_ref.digest_words(words) == want, words
    assert digest_ref.digest(np.arange(1000, dtype=np.float32)) == digest_ref.KNOWN_ARANGE_1000_F32
    words = list(range(7, 40))
    prefixes = digest_ref.prefix_digests(words, [1, 5, 33])
    assert prefixes == {n: digest_ref.digest_words(words[:n]) for n in (1, 5, 33)}


def test_digest_host_known_answers():
    from generative_models_amd.checkpoint import digest_host
    for words, want in digest_ref.KNOWN:
        assert digest_host(np.array(words, dtype=np.uint32)) == want, words
    assert digest_host(np.arange(1000, dtype=np.float32)) == digest_ref.KNOWN_ARANGE_1000_F32
    assert digest_host(torch.arange(1000, dtype=torch.float32)) == digest_ref.KNOWN_ARANGE_1000_F32


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 100003])
def test_digest_host_equals_the_reference(n):
    from generative_models_amd.checkpoint import digest_host
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    assert digest_host(a) == digest_ref.digest(a)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)      # every bit pattern, NaNs among them
    assert digest_host(w) == digest_ref.digest(w)
    assert digest_host(w.view(np.float32)) == digest_ref.digest(w)


def test_digest_host_spans_chunks_and_takes_other_dtypes():
    from generative_models_amd import checkpoint
    n = checkpoint._CHUNK + 5
    w = np.random.default_rng(0).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert checkpoint.digest_host(w) == digest_ref.digest(w)
    b = w[:6].view(np.uint8)
    assert checkpoint.digest_host(b) == digest_ref.digest(w[:6]) == checkpoint.digest_host(w[:6].view(np.int64))
    with pytest.raises(ValueError):
        checkpoint.digest_host(np.zeros(6, dtype=np.uint8))
    with pytest.raises(ValueError):
        checkpoint.digest_host(np.zeros(0, dtype=np.float32))


def test_digest_host_sees_the_sign_of_zero_and_the_order():
    from generative_models_amd.checkpoint import digest_host
    a = np.zeros(16, dtype=np.float32)
    b = a.copy()
    b[5] = -0.0
    assert digest_host(a) != digest_host(b)
    c = np.arange(16, dtype=np.float32)
    d = c.copy()
    d[[2, 11]] = d[[11, 2]]
    assert digest_host(c) != digest_host(d)
    assert digest_host(c) == digest_host(c.copy())


# ---- header and binding --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_matches():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    ret, argtypes, argnames = protos["gmk_arena_digest"]
    assert argnames == ["data", "n_words", "out", "stream"] and ret is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    fn = _lib.lib.gmk_arena_digest
    assert list(fn.argtypes) == argtypes and fn.restype is ret
    assert _lib.PROTOS["gmk_arena_digest"] == protos["gmk_arena_digest"]


def test_entry_rejects_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(64)        # never dereferenced: argument checks come first
    assert lib.gmk_arena_digest(None, 8, buf, None) == -1 and b"null" in lib.gmk_last_error()
    assert lib.gmk_arena_digest(buf, 8, None, None) == -1 and b"null" in lib.gmk_last_error()
    assert lib.gmk_arena_digest(buf, 0, buf, None) == -1 and b"n_words" in lib.gmk_last_error()
    assert lib.gmk_arena_digest(buf, -4, buf, None) == -1 and b"n_words" in lib.gmk_last_error()
    assert lib.gmk_arena_digest(ctypes.c_void_p(66), 8, buf, None) == -1 and b"4-byte aligned" in lib.gmk_last_error()
    assert lib.gmk_arena_digest(buf, 8, ctypes.c_void_p(68), None) == -1 and b"8-byte aligned" in lib.gmk_last_error()


# ---- state round trips -----------------------------------------------------------------------------------------------------------------
def test_philox_stream_round_trip():
    from generative_models_amd.diffusion.gaussian_diffusion import PhiloxStream
    draws = [5, 1, 784 * 8, 3]
    a = PhiloxStream(1234)
    first = [a._take(n) for n in draws]                      # counters only: no launch
    saved = a.state_dict()
    assert saved == {"seed": 1234, "counter": a.counter} and a.counter == sum((n + 3) // 4 for n in draws)
    second = [a._take(n) for n in draws]
    b = PhiloxStream(1234)
    assert [b._take(n) for n in draws] == first              # a fresh stream starts over ...
    b.load_state_dict(saved)
    assert [b._take(n) for n in draws] == second             # ... a loaded one continues
    assert b.state_dict() == a.state_dict()
    with pytest.raises(ValueError, match="seed"):
        PhiloxStream(1235).load_state_dict(saved)


def _epoch(ds):
    return [(x.clone(), y.clone()) for x, y in ds]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(xa, xb) and torch.equal(ya, yb) for (xa, ya), (xb, yb) in zip(a, b))


def test_synthetic_mnist_round_trip_on_the_cpu():
    from generative_models_amd.data import SyntheticMNIST
    make = lambda: SyntheticMNIST(4, 3, 0, 0, "cpu", seed=7)
    a = make()
    first = _epoch(a)
    saved = a.state_dict()
    second = _epoch(a)
    assert not _same(first, second)
    b = make()
    assert _same(_epoch(b), first)
    b = make()
    b.load_state_dict(saved)
    assert _same(_epoch(b), second)
    a._counter = 17                                          # the device path's position travels too
    b.load_state_dict(a.state_dict())
    assert b._counter == 17


def test_mnist_loader_round_trip(tmp_path):
    from generative_models_amd import data
    rng = np.random.default_rng(0)
    raw = tmp_path / "MNIST" / "raw"
    raw.mkdir(parents=True)
    img, lab = data.FILES[True]
    data.write_idx(raw / img, rng.integers(0, 256, size=(24, 28, 28), dtype=np.uint8))
    data.write_idx(raw / lab, (np.arange(24) % 10).astype(np.uint8))
    make = lambda: data.MnistLoader(str(tmp_path), True, 4, binarize=False, seed=3)
    a = make()
    first = _epoch(a)
    saved = a.state_dict()
    second = _epoch(a)
    assert len(first) == 6 and not _same(first, second)
    b = make()
    b.load_state_dict(saved)
    assert _same(_epoch(b), second)
    assert _same(_epoch(make()), first)


def test_device_dataset_state_is_epoch_and_k():
    """DeviceDataset lives on a GPU; its state methods are plain attribute moves, checked here on an object built without its constructor."""
    from generative_models_amd.data import DeviceDataset
    a = object.__new__(DeviceDataset)
    a.epoch, a._k = 3, 12
    assert a.state_dict() == {"epoch": 3, "k": 12}
    b = object.__new__(DeviceDataset)
    b.load_state_dict(a.state_dict())
    assert (b.epoch, b._k) == (3, 12)


def test_fused_adam_state_carries_ema_seeded_and_survives_no_moments():
    m = _model(ema_decay=0.999)
    opt = m.optimizer
    sd = opt.state_dict()
    assert sd["m"] is None and sd["v"] is None and sd["ema_seeded"] is False and sd["step"] == 0 and sd["skipped"] == 0
    opt.seed_ema()
    opt.step_count = 9
    sd = opt.state_dict()
    assert sd["ema_seeded"] is True
    other = _model(ema_decay=0.999).optimizer
    other.load_state_dict(sd)
    assert other.m is None and other.v is None and other.ema_seeded and other.step_count == 9
    n = m.net.flat_params.numel()
    sd = dict(sd, m=torch.full((n,), 0.5), v=torch.full((n,), 0.25))
    other.load_state_dict(sd)
    assert other.m.device == m.net.flat_params.device and torch.equal(other.m, sd["m"]) and torch.equal(other.v, sd["v"])
    with pytest.raises(ValueError, match="'v'"):
        other.load_state_dict(dict(sd, v=torch.zeros(n - 4)))
    with pytest.raises(ValueError, match="'m'"):
        other.load_state_dict(dict(sd, m=torch.zeros(n + 4)))
    # a state dict from before the key existed keeps what the optimiser has
    other.load_state_dict({"step": 4, "m": None, "v": None, "lr": 1e-3, "skipped": 2})
    assert other.ema_seeded and other.step_count == 4 and other.state_dict()["skipped"] == 2


def _cpu_run():
    from generative_models_amd.data import SyntheticMNIST
    torch.manual_seed(0)
    model = _model(ema_decay=0.999, dropout=0.1)
    return model, SyntheticMNIST(4, 2, 0, 0, "cpu", seed=1000), SyntheticMNIST(4, 1, 0, 0, "cpu", seed=2000)


def test_model_train_state_round_trip_on_the_cpu(tmp_path):
    from generative_models_amd import checkpoint
    model, train_ds, test_ds = _cpu_run()
    n = model.net.flat_params.numel()
    model.optimizer.seed_ema()
    model.optimizer.m, model.optimizer.v = torch.rand(n), torch.rand(n)
    model.optimizer.step_count = 11
    model.diffusion.rng._take(100)
    model._aux_rng._take(36)
    model.net._drop_counter = 77
    _epoch(train_ds)
    torch.save(model.state_dict(), tmp_path / "model.pt")
    path = checkpoint.save(tmp_path, model, train_ds, test_ds, 4)
    assert path == tmp_path / "train_state.pt" and sorted(p.name for p in tmp_path.iterdir()) == ["model.pt", "train_state.pt"]
    record = torch.load(path, map_location="cpu")
    assert record["version"] == checkpoint.FORMAT_VERSION and record["epoch"] == 4 and record["world"] == 1
    assert set(record) == {"version", "epoch", "world", "model", "train_data", "test_data", "digests"}
    assert record["digests"] == record["model"]["digests"] == model.arena_digests()
    assert record["digests"]["params"] == checkpoint.digest_host(model.net.flat_params.numpy())
    next_epoch = _epoch(train_ds)

    _, train2, test2 = _cpu_run()
    torch.manual_seed(5)                                     # other initial weights
    fresh = _model(ema_decay=0.999, dropout=0.1)
    assert not torch.equal(fresh.net.flat_params, model.net.flat_params)
    fresh.load_state_dict(torch.load(tmp_path / "model.pt"))
    assert checkpoint.load(tmp_path, fresh, train2, test2) == 4
    opt = fresh.optimizer
    assert torch.equal(opt.m, model.optimizer.m) and torch.equal(opt.v, model.optimizer.v) and opt.step_count == 11 and opt.ema_seeded
    assert torch.equal(fresh.net.flat_params, model.net.flat_params) and torch.equal(fresh.ema_net.flat_params, model.ema_net.flat_params)
    assert fresh.diffusion.rng.counter == 25 and fresh._aux_rng.counter == 9 and fresh.net._drop_counter == 77
    assert fresh.arena_digests() == model.arena_digests()
    assert _same(_epoch(train2), next_epoch)


def test_a_state_before_the_first_step_round_trips(tmp_path):
    from generative_models_amd import checkpoint
    model, train_ds, test_ds = _cpu_run()
    torch.save(model.state_dict(), tmp_path / "model.pt")
    checkpoint.save(tmp_path, model, train_ds, test_ds, 0)
    record = torch.load(tmp_path / "train_state.pt", map_location="cpu")
    assert record["digests"]["m"] is None and record["digests"]["v"] is None and record["model"]["optimizer"]["m"] is None
    fresh = _model(ema_decay=0.999, dropout=0.1)
    fresh.load_state_dict(torch.load(tmp_path / "model.pt"))
    assert checkpoint.load(tmp_path, fresh, *_cpu_run()[1:]) == 0 and fresh.optimizer.m is None


def test_weights_of_another_checkpoint_are_refused(tmp_path):
    """model.pt and train_state.pt from different checkpoints: the parameter digest does not match, and nothing is loaded."""
    from generative_models_amd import checkpoint
    model, train_ds, test_ds = _cpu_run()
    model.optimizer.step_count = 3
    checkpoint.save(tmp_path, model, train_ds, test_ds, 1)
    other = _model(ema_decay=0.999, dropout=0.1)
    other.load_state_dict(model.state_dict())
    with torch.no_grad():
        other.net.flat_params[10] += 1.0                     # "a later checkpoint's weights"
    assert checkpoint.digest_host(other.net.flat_params) != checkpoint.digest_host(model.net.flat_params)
    with pytest.raises(RuntimeError, match="different checkpoints"):
        checkpoint.load(tmp_path, other, train_ds, test_ds)
    assert other.optimizer.step_count == 0
    ema_off = other
    ema_off.net.flat_params.copy_(model.net.flat_params)
    with torch.no_grad():
        ema_off.ema_net.flat_params[3] -= 1.0
    with pytest.raises(RuntimeError, match="'ema'"):
        checkpoint.load(tmp_path, ema_off, train_ds, test_ds)


# ---- flags -------------------------------------------------------------------------------------------------------------------------------
def _saved_run(tmp_path, extra=(), **record):
    """A directory as a run leaves it, as far as the flag layers read it: hps.yaml (from the flags of `extra`, plus `record` keys)."""
    from generative_models_amd import main
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--logdir", str(tmp_path), "--epochs", "1", "--bs", "8", *extra])
    G.full_cmd = "python -m generative_models_amd.main"
    G.update(record)
    run = Path(G.logdir)
    run.mkdir(parents=True, exist_ok=True)
    (run / "hps.yaml").write_text(yaml.dump(dict(G), width=float("inf")))
    return run


def test_flags_parse_and_default_to_off():
    from generative_models_amd import main
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.save_state == 0 and G.resume == Path(".") and type(main.DG.save_state) is int
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--save_state", "1"])
    assert G.save_state == 1 and G.resume == Path(".")


def test_resume_reads_the_saved_flags_under_the_command_line(tmp_path):
    from generative_models_amd import main
    run = _saved_run(tmp_path, ["--lr_warmup", "4", "--ema_decay", "0.999"])
    G, Model = main.FlagSpace(main.DG).resolve(["--resume", str(run)])
    assert G.resume == run and G.logdir == run and G.save_state == 1 and G.model == "diffusion" and Model.__name__ == "DiffusionModel"
    assert (G.epochs, G.bs, G.lr_warmup, G.ema_decay) == (1, 8, 4, 0.999) and "full_cmd" not in G
    G, _ = main.FlagSpace(main.DG).resolve(["--resume", str(run), "--epochs", "100", "--save_state", "0"])
    assert G.epochs == 100 and G.bs == 8 and G.save_state == 1          # the command line wins over hps.yaml; save_state is forced


def test_a_resume_key_in_hps_yaml_does_not_start_a_resume(tmp_path):
    from generative_models_amd import main
    run = _saved_run(tmp_path, resume=Path("/some/earlier/dir"), save_state=1)
    G, _ = main.FlagSpace(main.DG).resolve(["--weights_from", str(run / "model.pt")])
    assert G.resume == Path(".") and G.save_state == 1 and G.weights_from == run / "model.pt"
    G, _ = main.FlagSpace(main.DG).resolve(["--resume", str(run)])
    assert G.resume == run and G.logdir == run


# ---- error paths of --resume ---------------------------------------------------------------------------------------------------------
def test_resume_with_weights_from_is_refused(tmp_path):
    from generative_models_amd import main
    run = _saved_run(tmp_path)
    with pytest.raises(ValueError, match="--weights_from"):
        main.load_model_and_data(["--resume", str(run), "--weights_from", str(run / "model.pt")])


def test_resume_without_a_state_file_names_it(tmp_path):
    from generative_models_amd import main
    run = _saved_run(tmp_path)
    with pytest.raises(ValueError, match="train_state.pt") as err:
        main.load_model_and_data(["--resume", str(run)])
    assert "--save_state 1" in str(err.value)


@pytest.mark.parametrize("record, argv, match", [
    (dict(version=99, epoch=0, world=1), [], "format version 99"),
    (dict(epoch=0, world=1), [], "format version None"),
    (dict(version=1, epoch=0, world=2), [], "2 rank"),
    (dict(version=1, epoch=1, world=1), [], "--epochs"),
    (dict(version=1, epoch=7, world=1), ["--epochs", "7"], "--epochs"),
])
def test_resume_refuses_a_state_it_cannot_continue(tmp_path, record, argv, match):
    """Unknown format, another world size, nothing left to train: named before a model is built (the records hold nothing else)."""
    from generative_models_amd import main
    run = _saved_run(tmp_path)
    torch.save(record, run / "train_state.pt")
    with pytest.raises((ValueError, RuntimeError), match=match):
        main.load_model_and_data(["--resume", str(run), *argv])


def test_save_state_flag_is_zero_or_one(tmp_path):
    from generative_models_amd import main
    with pytest.raises(ValueError, match="--save_state"):
        main.load_model_and_data(["--model=diffusion", "--logdir", str(tmp_path), "--save_state", "2"])
