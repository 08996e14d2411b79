"""PowerSGD restated on the CPU in torch, in float64 (the reference of test_gpu_powersgd.py) or float32 (the
yardstick: what the same arithmetic costs in single precision). Per step and compressed tensor, seen as a row-major
rows x cols matrix, with c = 1 / world and rank w's gradient g_w already divided by the world size:

    A_w = g_w + e_w ;  Qh = mgs(Q) ;  P = sum_w A_w Qh ;  Ph = mgs(P) ;  Q = sum_w A_w^T Ph
    gh  = Ph Q^T    ;  e_w = A_w - c * gh

mgs is modified Gram-Schmidt dividing by (norm + eps); a column with norm + eps == 0 becomes zero, and a column whose
norm fell to 2^-20 of what it was before the projections (it lay in the span of its predecessors: what is left is
rounding noise) is divided by that earlier norm instead, so the noise stays negligible. Q starts as
torch.randn(total Q elements) drawn on the CPU in float32 from the seed, each tensor's block a row-major cols x rank
matrix; later steps start from the previous step's Q. Rank-0 tensors are summed over the ranks. If any P or Q of a
step is not finite, every compressed tensor's gh is NaN and e and Q stay as they were."""
import torch


DEPENDENT = 2.0 ** -20


def mgs(m, eps=0.0):
    m = m.clone()
    for k in range(m.shape[1]):
        before = m[:, k].norm()
        for j in range(k):
            m[:, k] -= (m[:, j] @ m[:, k]) * m[:, j]
        after = m[:, k].norm()
        den = (before if after <= DEPENDENT * before else after) + eps
        m[:, k] = torch.zeros_like(m[:, k]) if den == 0 else m[:, k] / den
    return m


class PowerSGDRef:
    def __init__(self, tensors, world, seed=0, dtype=torch.float64, eps=0.0, error_feedback=True):
        """tensors: (offset, rows, cols, rank) in offset order, rank 0 = uncompressed"""
        self.tensors, self.world, self.dtype, self.eps, self.ef = list(tensors), world, dtype, eps, error_feedback
        n_q = sum(c * k for _, _, c, k in self.tensors)
        init = torch.randn(n_q, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).to(dtype)
        self.q, off = [], 0
        for _, _, c, k in self.tensors:
            self.q.append(init[off:off + c * k].view(c, k).clone() if k else None)
            off += c * k
        self.e = [[torch.zeros(r, c, dtype=dtype) if k else None for _, r, c, k in self.tensors] for _ in range(world)]
        self.last_bad = False

    def step(self, grads):
        """grads: one flat float32 tensor per rank. Returns {tensor index: result} -- gh (rows x cols) for a
        compressed tensor, the sum over the ranks (flat) for the others -- and updates e and Q."""
        assert len(grads) == self.world
        out, new_q, new_e, bad = {}, {}, {}, False
        for i, (o, r, c, k) in enumerate(self.tensors):
            gs = [g[o:o + r * c].to(self.dtype) for g in grads]
            if k == 0:
                out[i] = sum(gs[1:], gs[0].clone())
                continue
            a = [g.view(r, c) + self.e[w][i] if self.ef else g.view(r, c) for w, g in enumerate(gs)]
            qh = mgs(self.q[i], self.eps)
            p = sum(x @ qh for x in a)
            ph = mgs(p, self.eps)
            q = sum(x.t() @ ph for x in a)
            gh = ph @ q.t()
            bad = bad or not bool(torch.isfinite(p).all() and torch.isfinite(q).all())
            out[i], new_q[i] = gh, q
            new_e[i] = [x - gh / self.world for x in a]
        self.last_bad = bad
        for i in new_q:
            if bad:
                out[i] = torch.full_like(out[i], float("nan"))
            else:
                self.q[i] = new_q[i]
                if self.ef:
                    for w in range(self.world):
                        self.e[w][i] = new_e[i][w]
        return out
