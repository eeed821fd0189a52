"""The differentiable weighted tanh-SP decoder of include/ldpc_abi.h ("Training") in plain torch on the CPU, from
``Graph`` indices: gather, exclusive products by explicit loops over slots, ``torch.clamp``, ``index_add``.  Its
gradients are ``torch.autograd``'s.  float64 is the reference; the same code in float32 is the fp32 yardstick."""
import numpy as np
import torch


class Ref:
    def __init__(self, g):
        self.g = g
        tgt, src, pos = g.vn_weight_index()   # off-diagonal (target var-order slot, source edge, compact position)
        self.tgt, self.src, self.pos = (torch.from_numpy(a) for a in (tgt, src, pos))
        self.vs = torch.from_numpy(np.repeat(np.arange(g.n), g.var_degrees()))   # variable of a var-order slot
        self.ve = torch.from_numpy(np.asarray(g.var_edges, np.int64))            # its check-order edge
        self.inv = torch.argsort(self.ve)                                        # edge -> var-order slot
        dc = g.check_degrees()
        idx = np.full((g.m, int(dc.max())), g.E, np.int64)                       # padded with a column of ones
        for c in range(g.m):
            idx[c, :dc[c]] = np.arange(g.row_ptr[c], g.row_ptr[c + 1])
        self.idx, self.valid = torch.from_numpy(idx), torch.from_numpy(idx < g.E)

    def forward(self, llr, w, iters, clamp=10.0, soft="p1"):
        """llr (B, n), w = dict(vn (iters, W), llr (iters, n), fin (E,), fin_llr (n,)) of one dtype ->
        (soft (B, n), |y| (B, E) of the last iteration before the message clamp)."""
        g, B = self.g, llr.shape[0]
        L = -llr
        x = torch.zeros(B, g.E, dtype=llr.dtype, device=llr.device)
        for it in range(iters):
            s = (w["llr"][it] * L)[:, self.vs]
            s = 0.5 * s.index_add(1, self.tgt, w["vn"][it][self.pos] * x[:, self.src])
            tau = torch.cat([torch.tanh(s)[:, self.inv], torch.ones(B, 1, dtype=llr.dtype, device=llr.device)], 1)[:, self.idx]
            D = tau.shape[2]
            p = []
            for k in range(D):            # exclusive products, slot by slot: no division by tau
                q = torch.ones_like(tau[:, :, 0])
                for j in range(D):
                    if j != k:
                        q = q * tau[:, :, j]
                p.append(q)
            p = torch.clamp(torch.stack(p, 2), -(1 - 1e-7), 1 - 1e-7)
            y = torch.log((1 + p) / (1 - p))[:, self.valid]
            x = torch.clamp(y, -clamp, clamp)
        z = (w["fin_llr"] * L).index_add(1, self.vs, w["fin"] * x[:, self.ve])
        z = 0.5 * z
        return (z if soft == "z" else 1 - torch.sigmoid(z)), y.detach().abs()

    def grads(self, llr, w, G, iters, clamp=10.0, soft="p1", dtype=torch.float64):
        """dict(vn, llr_w, fin, fin_llr, llr) of d sum(G * soft), plus soft and the last |y|, evaluated in dtype."""
        t = {k: torch.as_tensor(v).to(dtype).requires_grad_() for k, v in dict(w, x=llr).items()}
        sft, y = self.forward(t["x"], t, iters, clamp, soft)
        (sft * torch.as_tensor(G).to(dtype)).sum().backward()
        out = {k: t[s].grad.double().numpy() for k, s in
               (("vn", "vn"), ("llr_w", "llr"), ("fin", "fin"), ("fin_llr", "fin_llr"), ("llr", "x"))}
        return dict(out, soft=sft.detach().double().numpy(), y=y.double().numpy())
