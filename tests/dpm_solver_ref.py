"""CPU restatement of sampler='dpmpp_2m' (DPM-Solver++(2M), Lu et al. 2022, Algorithm 2, data prediction) - test infrastructure.

Built on the oracle's reference pieces: the prediction of each step is `run_model` (+ `cf_guidance`) exactly as the DDIM step forms it, on
DDIM's time grid (`sampler_times`, `logsnr_schedule_cosine`).  The solver's coefficients are computed here in float64 from the fp32
log-SNRs, independently of the package's `dpm_solver_coefs`:
    lambda = logsnr / 2, alpha = sqrt(sigmoid(logsnr)), sigma = sqrt(sigmoid(-logsnr)), h = lambda_s - lambda_t
    first step:  z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) x_hat
    later steps: D = (1 + 1/(2r)) x_hat - 1/(2r) x_hat_prev, r = h_prev / h;  z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D
    last step:   z = x_hat
The recorded trajectory is (z, x_hat, eps_hat) - the prediction, not D."""
import sampler_ref as S


def sample(params, init_x, guide, num_steps, cond_w=None, mean_type="v", record=True):
    """-> (zs, xs, es) stacked [T, B, ...] when `record`, else the final z.  `cond_w`: resolved per-sample guidance weights or None."""
    return S.chain(init_x, num_steps, S.oracle_step(params, guide, "dpmpp_2m", cond_w, mean_type), record=record)
