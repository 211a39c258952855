"""CPU tests (no GPU) of DDNM restoration (`GaussianDiffusion.restore`, `DiffusionModel.degrade` / `restore`, gmk_box_mean, gmk_box_residual,
gmk_sampler_step_ns, gmk_dpm_solver_step_ns, DG.restore_eval / DG.restore_gray; an extension): the algebra of the restatement
(tests/restore_ref.py) - A A+ = I, the projection and its idempotence, A(x + A+(y - A x)) = y, the fp32 emulation's rounding bound - the
restatement's anchor to the oracle's DDIM chain, option validation, the C ABI and its argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restore_ref as R  # noqa: E402

# (C, H, W, cf, N): the kernel shapes of tests/test_gpu_restore.py
SHAPES = [(1, 8, 8, 1, 2), (3, 8, 8, 3, 1), (3, 8, 8, 3, 2), (1, 12, 12, 1, 3), (1, 28, 28, 1, 7), (3, 32, 32, 1, 2), (3, 32, 32, 1, 8)]
U24 = 2.0 ** -24


def _rand(shape, seed, dtype=torch.float64):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype) * 2 - 1


@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_operator_algebra(C, H, W, cf, N):
    B = 3
    x = _rand((B, C, H, W), 1)
    u = _rand((B, C // cf, H // N, W // N), 2)
    assert R.A(x, cf, N).shape == u.shape and R.A_pinv(u, cf, N).shape == x.shape
    # A is the mean over the members the issue lists: element (c' cf + dc, i N + dy, j N + dx) belongs to box (c', i, j)
    idx = R.box_index((C, H, W), cf, N)
    want = torch.zeros((B, u[0].numel()), dtype=torch.float64).index_add_(1, idx.flatten(), x.flatten(1)) / (cf * N * N)
    assert torch.allclose(R.A(x, cf, N).flatten(1), want, rtol=0, atol=1e-15)
    assert torch.equal(R.A_pinv(u, cf, N).flatten(1), u.flatten(1)[:, idx.flatten()])
    # A A+ = I (replication, then a mean of equal values: exact up to the mean's own rounding)
    assert float((R.A(R.A_pinv(u, cf, N), cf, N) - u).abs().max()) <= 1e-15
    # the projection lands on {x : A x = y} and is idempotent
    p = R.project(x, u, cf, N)
    assert float((R.A(p, cf, N) - u).abs().max()) <= 1e-15
    assert float((R.project(p, u, cf, N) - p).abs().max()) <= 1e-15
    # and it moves x along the range space only: the null-space part x - A+ A x is untouched
    null = lambda t: t - R.A_pinv(R.A(t, cf, N), cf, N)
    assert float((null(p) - null(x)).abs().max()) <= 1e-15


@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_fp32_emulation_meets_the_bounds(C, H, W, cf, N):
    """The kernel arithmetic restated in numpy fp32: the box mean within (k + 1) 2^-24 of float64 for inputs in [-1, 1], and the projected
    x-hat' = fadd(x_hat, fsub(obs, mean)) within (k + 4) 2^-24 of obs under a float64 A - the bars of the GPU tests."""
    k = cf * N * N
    x = _rand((3, C, H, W), 3, torch.float32)
    m = R.box_mean_fp32(x, cf, N)
    assert float(np.abs(m.astype(np.float64) - R.A(x.double(), cf, N).numpy()).max()) <= (k + 1) * U24
    obs = R.box_mean_fp32(_rand((3, C, H, W), 4, torch.float32), cf, N)
    r = (obs - m).astype(np.float32)
    xp = (x.numpy() + R.A_pinv(torch.from_numpy(r), cf, N).numpy()).astype(np.float32)
    got = R.A(torch.from_numpy(xp).double(), cf, N).numpy()
    assert float(np.abs(got - obs.astype(np.float64)).max()) <= (k + 4) * U24


def test_restatement_chain_and_its_anchor_to_the_oracle():
    """Every step's x-hat' of the restating chain, and so its end, satisfies A x = obs; the x-hat it projects is the oracle's (C = 32 keeps
    the CPU U-Net fast)."""
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    params = U.reference_init_params(32, 1, zero_out_layers=False, seed=3)
    g = torch.Generator().manual_seed(4)
    init = torch.randn((2, 1, 8, 8), generator=g)
    y = torch.tensor([2, 5])
    obs = R.A(_rand((2, 1, 8, 8), 5), 1, 2)
    with torch.no_grad():
        for sampler in ("ddim", "dpmpp_2m"):
            zs, xs, es = R.sample(params, init, obs, 1, 2, y, 4, sampler)
            assert float((R.A(zs[-1], 1, 2) - obs).abs().max()) <= 1e-14
            assert float((R.A(xs.flatten(0, 1), 1, 2) - obs.repeat(4, 1, 1, 1)).abs().max()) <= 1e-14           # every step's x-hat' agrees with the observation
            assert float(xs.abs().max()) <= 3.0
        # x_hat() is the oracle's prediction: run_model's clip, and cf_guidance between two clips (fp32 there, float64 here)
        z = torch.randn((2, 1, 8, 8), generator=g)
        w = torch.tensor([0.5, 2.0])
        for mean_type in ("v", "eps", "x"):
            for l in (-3.0, 1.0):
                lt = torch.full((2,), l)
                out = U.unet_forward(params, z, lt, guide=y)
                out_u = U.unet_forward(params, z, lt, guide=-torch.ones_like(y))
                want = D.model_outputs(out, z, lt, mean_type)
                assert float((R.x_hat(out, z, lt, mean_type) - want["model_x"]).abs().max()) <= 1e-5
                want_g = D.cf_guidance(params, z, want["model_eps"], lt, w, y, mean_type)[0]
                assert float((R.x_hat(out, z, lt, mean_type, out_u, w) - want_g).abs().max()) <= 1e-4
        noises = [torch.randn((2, 1, 8, 8), generator=g) for _ in range(4)]
        zs = R.sample(params, init, obs, 1, 2, y, 4, "noisy", noises=noises)[0]
        assert float((R.A(zs[-1], 1, 2) - obs).abs().max()) <= 1e-14


def test_validation_errors():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, restore_operator
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    net = object()
    init3, init1 = torch.zeros((2, 3, 8, 8)), torch.zeros((2, 1, 8, 8))
    assert restore_operator((2, 3, 8, 8), 2, False) == (1, 2, (2, 3, 4, 4))
    assert restore_operator((2, 3, 8, 8), 1, True) == (3, 1, (2, 1, 8, 8))
    assert restore_operator((2, 3, 8, 8), 4, True) == (3, 4, (2, 1, 2, 2))
    with pytest.raises(ValueError, match="k = cf factor"):                       # k < 2
        d.restore(net=net, obs=init3, factor=1, gray=False, init_x=init3)
    with pytest.raises(ValueError, match="one channel"):                         # gray with C == 1
        d.restore(net=net, obs=init1, gray=True, init_x=init1)
    with pytest.raises(ValueError, match="obs shape"):                           # obs of the wrong shape
        d.restore(net=net, obs=torch.zeros((2, 3, 4, 2)), factor=2, init_x=init3)
    with pytest.raises(ValueError, match="obs shape"):
        d.restore(net=net, obs=torch.zeros((2, 3, 4, 4)), factor=2, gray=True, init_x=init3)
    with pytest.raises(ValueError, match="does not divide"):
        d.restore(net=net, obs=torch.zeros((2, 3, 2, 2)), factor=3, init_x=init3)
    for bad in (0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="factor"):
            d.restore(net=net, obs=init3, factor=bad, init_x=init3)
    with pytest.raises(ValueError, match="teacher_test"):
        GaussianDiffusion(mean_type="v", num_steps=4, sampler="teacher_test").restore(net=net, obs=init1[..., ::2, ::2], factor=2, init_x=init1)
    with pytest.raises(ValueError, match="out of scope"):                        # dynamic thresholding
        GaussianDiffusion(mean_type="v", num_steps=4, dyn_threshold=0.995).restore(net=net, obs=init1[..., ::2, ::2], factor=2, init_x=init1)
    from generative_models_amd.diffusion.gaussian_diffusion import InpaintState, RestoreState
    with pytest.raises(ValueError, match="out of scope"):                        # together with inpainting
        d._sample(net=net, init_x=init1, inp=InpaintState(None, None, None, 1, 2, []), rst=RestoreState(None, 1, 2))


def test_ops_geometry_errors():
    from generative_models_amd import ops
    assert ops.box_geometry((2, 3, 8, 8), 3, 2) == (2, 3, 8, 8, 3, 2, (2, 1, 4, 4))
    for shape, cf, N, word in (((2, 3, 8, 8), 2, 2, "cf"), ((2, 3, 8, 8), 1, 3, "divide"), ((2, 3, 8, 12), 1, 8, "divide"), ((2, 3, 8, 8), 1, 0, "divide"),
                               ((3, 8, 8), 1, 2, "shape"), ((2, 3, 8, 8), 1.5, 2, "integers"), ((40000, 3, 256, 256), 1, 1, "2\\^31")):
        with pytest.raises(ValueError, match=word):
            ops.box_geometry(shape, cf, N)


def test_defaults_and_flags():
    from generative_models_amd import common, main
    Model = common.discover_models()["diffusion_model"]
    assert Model.DG.restore_eval == 0 and Model.DG.restore_gray == 0
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.restore_eval == 0 and G.restore_gray == 0
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--restore_eval", "4", "--restore_gray", "1"])
    assert G.restore_eval == 4 and G.restore_gray == 1

    def build(**flags):
        G = common.AttrDict(dict(Model.DG))
        G.update(lr=3e-4, pad32=0, device="cpu", timesteps=4, bs=8)
        G.update(flags)
        return Model(G)
    for flags, word in (({"restore_eval": 1}, "restore_eval"), ({"restore_eval": -2}, "restore_eval"), ({"restore_gray": 2}, "restore_gray"),
                        ({"restore_gray": 1}, "in_channels"), ({"restore_eval": 2, "dyn_threshold": 0.9}, "out of scope")):
        with pytest.raises(ValueError, match=word):
            build(**flags)
    assert Model.RESTORE_EVAL_SEED not in (Model.INPAINT_EVAL_SEED, Model.INPAINT_EVAL_SEED + 1, Model.EDIT_EVAL_SEED, 0)


def test_header_declares_the_entries():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    geom = ["C", "H", "W", "cf", "N"]
    assert protos["gmk_box_mean"] == (ctypes.c_int, [P, P] + [I] * 6 + [P], ["x", "out", "B"] + geom + ["stream"])
    assert protos["gmk_box_residual"] == (ctypes.c_int, [P] * 5 + [F, P] + [I] * 7 + [P],
                                          ["v", "v_uncond", "cond_w", "z", "obs", "logsnr_t", "r", "mean_type", "B"] + geom + ["stream"])
    # the _ns entries: the plain lists plus `r` after cond_w and the geometry before the stream
    for base in ("gmk_sampler_step", "gmk_dpm_solver_step"):
        ret, types, names = protos[base]
        assert protos[base + "_ns"] == (ret, types[:3] + [P] + types[3:-1] + [I] * 5 + [P], names[:3] + ["r"] + names[3:-1] + geom + ["stream"])


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def mean(x=buf, out=buf, B=2, C=3, H=8, W=8, cf=1, N=2):
        return lib.gmk_box_mean(x, out, B, C, H, W, cf, N, None)

    def res(v=buf, vu=None, w=None, z=buf, obs=buf, r=buf, lt=-1.0, mt=0, B=2, C=3, H=8, W=8, cf=1, N=2):
        return lib.gmk_box_residual(v, vu, w, z, obs, lt, r, mt, B, C, H, W, cf, N, None)

    def step(r=buf, v=buf, vu=None, w=None, z=buf, zn=buf, mt=0, B=2, n=192, C=3, H=8, W=8, cf=1, N=2):
        return lib.gmk_sampler_step_ns(v, vu, w, r, z, None, -1.0, 1.0, 0, zn, None, None, None, None, mt, B, n, C, H, W, cf, N, None)

    def dpm(r=buf, v=buf, vu=None, w=None, z=buf, hist=buf, zn=buf, mt=0, B=2, n=192, C=3, H=8, W=8, cf=1, N=2, coef_prev=0.5):
        return lib.gmk_dpm_solver_step_ns(v, vu, w, r, z, hist, -1.0, 1.0, 0.5, 0.5, coef_prev, 0, zn, None, None, None, None, mt, B, n, C, H, W,
                                          cf, N, None)
    for call in (mean, res, step, dpm):
        assert call(cf=2) == -1 and b"cf = 2" in lib.gmk_last_error()                      # cf not in {1, C}
        for kw in ({"N": 3}, {"N": 0}, {"W": 12, "N": 8}, {"H": 12, "N": 8}):              # N not dividing H or W
            assert call(**kw) == -1 and b"does not divide" in lib.gmk_last_error()
        assert call(B=0) == -1 and b"shape" in lib.gmk_last_error()
    # B n_box >= 2^31: 40000 x 3 x 256 x 256 at k = 1 is 7.9e9 boxes; the same images at cf = 3, N = 2 are 6.6e8 and pass the check
    for call in (mean, res):
        assert call(B=40000, H=256, W=256, N=1) == -1 and b"2^31" in lib.gmk_last_error()
    assert mean(x=None) == -1 and b"null pointer" in lib.gmk_last_error()
    for kw in ({"v": None}, {"z": None}, {"obs": None}, {"r": None}):
        assert res(**kw) == -1 and b"null pointer" in lib.gmk_last_error()
    assert res(mt=3) == -1 and b"mean_type" in lib.gmk_last_error()
    assert res(vu=buf) == -1 and b"together" in lib.gmk_last_error()
    assert res(lt=float("nan")) == -1 and b"non-finite" in lib.gmk_last_error()
    for call in (step, dpm):
        for kw in ({"r": None}, {"v": None}, {"z": None}, {"zn": None}):
            assert call(**kw) == -1 and b"null pointer" in lib.gmk_last_error()
        assert call(n=191) == -1 and b"is not C H W" in lib.gmk_last_error()
        assert call(mt=3) == -1 and b"mean_type" in lib.gmk_last_error()
        assert call(vu=buf) == -1 and b"together" in lib.gmk_last_error()
    assert b"gmk_dpm_solver_step_ns" in lib.gmk_last_error()                               # errors name the entry that was called
