"""Resumable training on the GPU: ops.arena_digest (HIP) against the pure-Python restatement tests/digest_ref.py, a model that is saved,
rebuilt and continued against the one that never stopped (graphed and kernel-by-kernel step), the driver's --save_state / --resume end to end
in fresh processes, its error paths, and the replica check in a one-rank RCCL group.  Every comparison is bit-exact."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_ref  # noqa: E402

# ---- the digest ------------------------------------------------------------------------------------------------------------------------
# One pass of the kernel's grid (1024 workgroups x 256 lanes x 4 words) covers 2^20 words: 2^20 + 3 is one full pass plus a tail, 2^23 + 5
# is eight passes of the grid-stride loop plus a quad and a one-word tail.
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 2 ** 20 + 3, 2 ** 23 + 5]
INT64_COUNTS = [1, 3, 4, 5, 255, 256, 257, 2 ** 19 + 3, 2 ** 22 + 2]          # 8-byte elements: twice as many words each


@pytest.fixture(scope="module")
def words():
    """(device int32 tensor of 2^23 + 5 random words - every bit pattern, NaNs among them -, {n: reference digest of the first n words}): the
    reference loop runs ONCE over the buffer, every test below reads a prefix of it."""
    host = np.random.default_rng(0).integers(0, 1 << 32, size=max(LENGTHS), dtype=np.uint64).astype(np.uint32)
    ref = digest_ref.prefix_digests(host.tolist(), set(LENGTHS) | {2 * m for m in INT64_COUNTS})
    return torch.from_numpy(host.view(np.int32)).cuda(), ref


@pytest.mark.parametrize("n", LENGTHS)
def test_digest_of_fp32_tensors(words, n):
    from generative_models_amd import ops
    dev, ref = words
    t = dev[:n].view(torch.float32)
    assert t.data_ptr() % 16 == 0
    got = ops.arena_digest(t)
    print(f"n = {n}: digest {got:#018x}, reference {ref[n]:#018x}")
    assert got == ref[n]
    assert ops.arena_digest(t) == got                                       # the entry zeroes its output: a second call gives the same value


@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_digest_of_a_view_off_the_16_byte_grid(words, n, start):
    """The same words behind a pointer that is 4-byte but not 16-byte aligned: `start` floats into a buffer."""
    from generative_models_amd import ops
    dev, ref = words
    buf = torch.zeros(n + start + 4, dtype=torch.int32, device="cuda")
    buf[start:start + n].copy_(dev[:n])
    t = buf[start:start + n].view(torch.float32)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * start
    assert ops.arena_digest(t) == ref[n]


@pytest.mark.parametrize("m", INT64_COUNTS)
def test_digest_of_int64_tensors(words, m):
    from generative_models_amd import ops
    dev, ref = words
    t = dev[:2 * m].view(torch.int64)
    assert t.numel() == m
    assert ops.arena_digest(t) == ref[2 * m]


@pytest.mark.parametrize("n", LENGTHS)
def test_digest_of_uint8_tensors(words, n):
    from generative_models_amd import ops
    dev, ref = words
    t = dev[:n].view(torch.uint8)
    assert t.numel() == 4 * n
    assert ops.arena_digest(t) == ref[n]


@pytest.mark.parametrize("n, word", [(1, 0), (257, 255), (2 ** 20 + 3, 2 ** 20 + 2), (2 ** 23 + 5, 2 ** 22 + 1), (2 ** 23 + 5, 2 ** 23 + 4)])
def test_one_flipped_bit_changes_the_digest(words, n, word):
    from generative_models_amd import ops
    dev, ref = words
    t = dev[:n].clone()
    assert ops.arena_digest(t) == ref[n]
    t[word] ^= 1 << 17
    flipped = ops.arena_digest(t)
    assert flipped != ref[n]
    t[word] ^= 1 << 17
    assert ops.arena_digest(t) == ref[n]
    if n > 1:                                                               # the position counts: two unequal words swapped
        other = 0 if word else 1
        a, b = int(t[word]), int(t[other])
        assert a != b
        t[word], t[other] = b, a
        assert ops.arena_digest(t) not in (ref[n], flipped)


def test_digest_does_not_follow_the_cu_limit(words):
    from generative_models_amd import ops
    from generative_models_amd._lib import lib
    dev, ref = words
    n = 2 ** 20 + 3
    before = lib.gmk_get_cu_limit()
    assert lib.gmk_set_cu_limit(64) == 0
    try:
        assert ops.arena_digest(dev[:n]) == ref[n]
    finally:
        assert lib.gmk_set_cu_limit(before) == 0


def test_digest_wrapper_and_host_function_agree(words):
    from generative_models_amd import checkpoint, ops
    dev, ref = words
    n = 2 ** 20 + 3
    assert checkpoint.digest_host(dev[:n].cpu()) == ref[n] == checkpoint.arena_digest(dev[:n])
    with pytest.raises(AssertionError):
        ops.arena_digest(dev[:8].cpu())
    with pytest.raises(AssertionError):
        ops.arena_digest(dev[:16:2])
    with pytest.raises(AssertionError):
        ops.arena_digest(dev[:2].view(torch.uint8)[:6])


# ---- in-process resume -----------------------------------------------------------------------------------------------------------------
def _model(dropout, seed):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=32, in_channels=1, image_size=8, ema_decay=0.999, grad_clip=1.0, lr_warmup=2, lr_scheduler="cosine", lr_decay_steps=5,
             dropout=dropout)
    torch.manual_seed(seed)
    return Model(G).cuda().train()


def _batches(k):
    g = torch.Generator().manual_seed(11)
    return [((torch.rand((8, 1, 8, 8), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()) for _ in range(k)]


def _steps(model, batches):
    out = []
    for x, y in batches:
        metrics = model.train_step(x, y.clone())
        out.append({k: metrics[k].detach().cpu().clone() for k in ("loss", "lr", "grad_norm", "skipped_steps")})
    torch.cuda.synchronize()
    return out


def _counters(model):
    return (model.diffusion.rng.state_dict(), model._aux_rng.state_dict(), model.net.dropout_state(), model.optimizer.step_count,
            model.optimizer.skipped_steps(), model.optimizer.ema_seeded)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_a_resumed_model_reaches_the_bits_of_the_one_that_never_stopped(tmp_path, dropout):
    """dropout 0: the step is the replayed graph; dropout 0.1: the kernel-by-kernel step, where the dropout counter is part of the state."""
    from generative_models_amd import ops
    batches = _batches(6)
    A = _model(dropout, 0)
    mA = _steps(A, batches)
    B = _model(dropout, 0)
    _steps(B, batches[:3])
    torch.save(B.state_dict(), tmp_path / "model.pt")
    torch.save(B.train_state(), tmp_path / "state.pt")
    del B

    C = _model(dropout, 1)                                                  # a fresh start under another seed: other initial weights
    assert not torch.equal(C.net.flat_params, A.net.flat_params)
    C.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    C.load_train_state(torch.load(tmp_path / "state.pt", map_location="cpu"))
    assert C.optimizer.m.is_cuda and C.optimizer.step_count == 3
    mC = _steps(C, batches[3:])
    assert ("_train_graphs" in C.__dict__) == (dropout == 0.0) == ("_train_graphs" in A.__dict__)
    if dropout > 0:
        assert A.net._drop_counter > 0
    for name, a, c in (("flat_params", A.net.flat_params, C.net.flat_params), ("m", A.optimizer.m, C.optimizer.m),
                       ("v", A.optimizer.v, C.optimizer.v), ("ema", A.ema_net.flat_params, C.ema_net.flat_params)):
        assert torch.equal(a, c), name
        assert ops.arena_digest(a) == ops.arena_digest(c), name
    assert A.arena_digests() == C.arena_digests()
    assert _counters(A) == _counters(C)
    for step, (a, c) in enumerate(zip(mA[3:], mC)):
        for key in a:
            assert torch.equal(a[key], c[key]), (step, key, a[key], c[key])

    # the control: the weights alone (what --weights_from loads) do NOT continue the run
    D = _model(dropout, 1)
    D.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    _steps(D, batches[3:])
    assert not torch.equal(D.net.flat_params, A.net.flat_params)
    assert ops.arena_digest(D.net.flat_params) != ops.arena_digest(A.net.flat_params)

    # and a train state is refused by weights it was not saved with
    with pytest.raises(RuntimeError, match="different checkpoints"):
        D.load_train_state(torch.load(tmp_path / "state.pt", map_location="cpu"))


# ---- the driver, in fresh processes ------------------------------------------------------------------------------------------------------
BASE = ["--model=diffusion", "--bs", "8", "--timesteps", "4", "--train_batches", "3", "--test_batches", "1", "--save_n", "1", "--save_state", "1",
        "--ema_decay", "0.999", "--lr_warmup", "4"]


def _driver(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "GMK_FORCE_EXCHANGE")}
    return subprocess.run([sys.executable, "-m", "generative_models_amd.main"] + [str(a) for a in argv], capture_output=True, text=True, timeout=600,
                          cwd=ROOT, env=dict(env, OMP_NUM_THREADS="2"))


def _ok(argv):
    r = _driver(argv)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _loss_lines(stdout):
    return [line for line in stdout.splitlines() if line.startswith("diffusion/train/loss ")]


def _same_values(a, b, where="state"):
    """Equality of two saved records: dicts and lists by element, tensors by torch.equal, everything else by ==."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), where
        for k in a:
            _same_values(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same_values(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), where
    else:
        assert a == b, (where, a, b)


def _three_runs(tmp, extra):
    """--epochs 2 straight through; --epochs 1, then --resume <dir> --epochs 2.  The driver does not seed torch's global generator, so two fresh
    starts draw different initial weights: both start from the weights an `--epochs 0` run of the same flags leaves (`--weights_from`, which a
    resumed run must not read again).  -> (straight dir, resumed dir, a copy of the resumed run's epoch-1 model.pt, the three stdouts)"""
    init, straight, split = tmp / "init", tmp / "straight", tmp / "split"    # a --logdir given on the command line is the run's directory as it is
    _ok(BASE + extra + ["--epochs", "0", "--logdir", init])
    start = BASE + extra + ["--weights_from", init / "model.pt"]
    out_straight = _ok(start + ["--epochs", "2", "--logdir", straight])
    out_first = _ok(start + ["--epochs", "1", "--logdir", split])
    shutil.copy(split / "model.pt", tmp / "model_epoch1.pt")
    assert torch.load(split / "train_state.pt", map_location="cpu")["epoch"] == 1
    (init / "model.pt").unlink()                                            # the resumed run takes its weights from its own directory
    out_resumed = _ok(["--resume", split, "--epochs", "2"])
    return straight, split, tmp / "model_epoch1.pt", (out_straight, out_first, out_resumed)


def _check_three_runs(straight, split, outs, steps):
    a, b = torch.load(straight / "model.pt", map_location="cpu"), torch.load(split / "model.pt", map_location="cpu")
    assert list(a) == list(b) and len(a) > 160                              # 160 keys of the net, and the EMA net's
    for key in a:
        assert torch.equal(a[key], b[key]), key
    sa, sb = torch.load(straight / "train_state.pt", map_location="cpu"), torch.load(split / "train_state.pt", map_location="cpu")
    assert sa["epoch"] == sb["epoch"] == 2 and sa["digests"] == sb["digests"] and sa["digests"]["m"] is not None
    assert sa["model"]["optimizer"]["step"] == steps and sa["model"]["rng"]["counter"] > 0 and sa["model"]["aux_rng"]["counter"] > 0
    _same_values(sa, sb)
    out_straight, out_first, out_resumed = outs
    lines = _loss_lines(out_straight)
    assert len(lines) == 2 and _loss_lines(out_first) == lines[:1]
    assert _loss_lines(out_resumed) == lines[1:]                            # character for character
    assert "RESUMED" in out_resumed and "RUNNING HEAVY EVAL" in out_straight    # eval_heavy stays at the model's default, 1
    return sa


@pytest.fixture(scope="module")
def synthetic_runs(tmp_path_factory):
    return _three_runs(tmp_path_factory.mktemp("resume_cli"), [])


def test_cli_resume_equals_the_straight_run(synthetic_runs):
    straight, split, _, outs = synthetic_runs
    state = _check_three_runs(straight, split, outs, steps=6)
    assert state["train_data"]["counter"] > 0 and state["test_data"]["counter"] > 0


def test_cli_resume_equals_the_straight_run_on_a_device_dataset(tmp_path):
    rng = np.random.default_rng(3)
    for split in ("train", "test"):
        np.save(tmp_path / f"{split}_images.npy", rng.integers(0, 256, size=(64, 1, 8, 8), dtype=np.uint8))
        np.save(tmp_path / f"{split}_labels.npy", (np.arange(64) % 10).astype(np.uint8))
    extra = ["--data", "npy", "--data_device", "1", "--flip_p", "0.5", "--image_size", "8", "--binarize", "0", "--data_root", tmp_path]
    straight, split, _, outs = _three_runs(tmp_path, extra)
    state = _check_three_runs(straight, split, outs, steps=16)
    # two epochs of 8 batches on the train split; the test split is walked once per evaluation and once per heavy evaluation
    assert state["train_data"] == {"epoch": 2, "k": 16} and state["test_data"]["epoch"] > 2


def test_resume_without_a_state_file_fails_by_name(synthetic_runs, tmp_path):
    straight = synthetic_runs[0]
    run = tmp_path / "run"
    shutil.copytree(straight, run)
    (run / "train_state.pt").unlink()
    r = _driver(["--resume", run, "--epochs", "3"])
    assert r.returncode != 0 and "train_state.pt" in r.stderr and "--save_state 1" in r.stderr, r.stderr[-3000:]


def test_resume_with_the_weights_of_another_checkpoint_fails_by_digest(synthetic_runs, tmp_path):
    """train_state.pt of epoch 2 beside the model.pt of epoch 1 - what a crash between the two writes leaves."""
    straight, _, model_epoch1, _ = synthetic_runs
    run = tmp_path / "run"
    shutil.copytree(straight, run)
    shutil.copy(model_epoch1, run / "model.pt")
    r = _driver(["--resume", run, "--epochs", "3"])
    assert r.returncode != 0 and "digest" in r.stderr and "different checkpoints" in r.stderr, r.stderr[-3000:]
    assert "diffusion/train/loss" not in r.stdout                           # refused before any training


# ---- the replica check, one rank ---------------------------------------------------------------------------------------------------------
_EXCHANGE_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from generative_models_amd import checkpoint, common, parallel
from generative_models_amd.data import SyntheticMNIST
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
assert dist.get_world_size() == 1 and parallel.exchanging()
Model = common.discover_models()["diffusion_model"]
G = common.AttrDict(dict(Model.DG))
G.update(hidden_size=32, in_channels=1, image_size=8, ema_decay=0.999)
torch.manual_seed(0)
model = Model(G).cuda().train()
g = torch.Generator().manual_seed(0)
x = (torch.rand((8, 1, 8, 8), generator=g) * 2 - 1).cuda(); y = torch.randint(0, 10, (8,), generator=g).cuda()
model.train_step(x, y)
calls = []
inner = parallel.check_replicas
def counted(digest, what, device, group=None):
    calls.append(inner(digest, what, device, group))
    return calls[-1]
parallel.check_replicas = counted
make = lambda seed: SyntheticMNIST(8, 1, 0, 0, "cuda", seed=seed)
path = checkpoint.save(sys.argv[2], model, make(1000), make(2000), 1)
digest = model.arena_digests()["params"]
assert calls == [[digest]], (calls, digest)
state = torch.load(path, map_location="cpu")
assert state["world"] == 1 and state["digests"]["params"] == digest and state["model"]["optimizer"]["step"] == 1
fresh = Model(G).cuda().train()
fresh.load_state_dict(model.state_dict())
assert checkpoint.load(sys.argv[2], fresh, make(1000), make(2000)) == 1 and fresh.arena_digests() == model.arena_digests()
dist.destroy_process_group()
print("replica check ok", hex(digest))
"""


def test_state_save_runs_the_replica_check_in_a_one_rank_group(tmp_path):
    import socket
    with socket.socket() as sock:                                           # a port nobody listens on right now
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port",
           port, str(script), ROOT, str(tmp_path / "run")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GMK_CU_LIMIT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=dict(env, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", GMK_FORCE_EXCHANGE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "replica check ok" in r.stdout
