"""C-PGD attack (stand-in for src/attacks/pgd/atk.py PGDTF2 on ART's
ProjectedGradientDescentTensorFlowV2): the whole loop runs in one kernel launch per batch
(mv_pgd_run).  Per iteration i on the scaled rows x (fp32):

  g = loss_gradient(x, y); NaN -> 0; g = 0 where mask == 0
  g = sign(g) (norm inf) | g / (||g||_2 + 1e-7) (norm 2)
  eta = eps_step, or eps * 10^-(i // (max_iter // 7) + 1) with "adaptive_eps_step"
  x = clip(x + eta g, 0, 1); d = x - x_init
  d = sign(d) min(|d|, eps) (inf) | d min(1, eps / (||d||_2 + 1e-7)) (2); x = x_init + d
  with "repair": x = scale(fix_features_types(unscale(x)))

Labels are the argmax of the model's own prediction on the clean rows; the result is the
last iterate.
"""
import numpy as np

from ..._native import norm_code
from .classifier import TF2Classifier, check_loss_evaluation, loss_flags


def adaptive_eps_step(eps: float, max_iter: int, i: int) -> float:
    """atk.py:129-132; max_iter < 7 divides by zero in the reference."""
    if max_iter < 7:
        raise ValueError(f"adaptive_eps_step needs max_iter >= 7 (got max_iter={max_iter})")
    power = np.float64(i // (max_iter // 7) + 1)
    return float(eps * (1 / np.float_power(10.0, power)))


class PGDTF2:
    def __init__(self, estimator: TF2Classifier, norm=np.inf, eps=0.3, eps_step=0.1,
                 max_iter=100, targeted=False, num_random_init=0, batch_size=32,
                 random_eps=False, tensor_board=False, verbose=True, loss_evaluation=""):
        if isinstance(norm, str) and norm.strip().lower() in ("inf", "np.inf"):
            norm = np.inf
        if not (norm == 2 or norm == np.inf):
            raise ValueError(f"norm {norm!r}: 2, np.inf or 'inf'")
        if num_random_init and int(num_random_init) > 0:
            raise ValueError("num_random_init > 0 (random restarts) is not supported")
        if targeted or random_eps:
            raise ValueError("targeted / random_eps are not supported")
        self.loss_evaluation = check_loss_evaluation(loss_evaluation)
        self.adaptive = "adaptive_eps_step" in self.loss_evaluation
        self.repair = "repair" in self.loss_evaluation
        self.max_iter = int(max_iter)
        if self.adaptive:
            adaptive_eps_step(float(eps), self.max_iter, 0)  # raises below 7
        self.estimator = estimator
        self.norm = norm
        self.eps = float(eps)
        self.eps_step = float(eps_step)
        self.batch_size = int(batch_size)

    def generate(self, x, y=None, mask=None):
        """x (n, D) scaled rows -> adversarial rows (n, D) float32.  ``mask`` must be the
        constraints' mutable mask (the one the driver passes) or None (the same)."""
        import torch

        est = self.estimator
        if mask is not None:
            m = np.asarray(mask).astype(bool)
            if m.shape != est.mutable_mask.shape:
                raise ValueError("mask: one entry per feature")
            if not (m == est.mutable_mask).all():
                if m.any():
                    raise ValueError("mask: the constraints' mutable mask (or all zero)")
                return np.array(x, dtype=np.float32, copy=True)  # nothing may move
        dev = torch.device("cuda", est.device)
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        out = np.empty_like(x)
        bs = max(self.batch_size, 1)
        for s in range(0, x.shape[0], bs):
            xd = torch.from_numpy(x[s:s + bs]).to(dev)
            yd = None
            if y is not None:
                yd = torch.from_numpy(np.ascontiguousarray(est._labels(y[s:s + bs]))).to(dev)
            xa = torch.empty_like(xd)
            est.pgd.run(xd, xa, self.max_iter, self.norm, self.eps, self.eps_step,
                        loss_flags(self.loss_evaluation), self.adaptive, self.repair, y=yd,
                        stream=torch.cuda.current_stream(dev))
            out[s:s + bs] = xa.cpu().numpy()
        return out
