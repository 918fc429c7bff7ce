"""The guarded batches and the case table of tests/test_gpu_gru_scan.py (shared with tools/gru_scan_probe.py): the scheme of
tests/td_targets_harness.py -- sentinel guard bands round every array, sentinel-filled outputs, NaN in the pitch padding of every
input -- for the two GRU scan launches."""
import itertools

import numpy as np
import torch

import gru_scan_twin as tw
from td_targets_harness import DEV, NAN, SENTINELS, guarded, guards_intact, words  # noqa: F401

FWD_OUT, BWD_OUT = ("h", "gates", "hidden_out"), ("dgi", "dghn", "d_hidden_in")


def draw_weights(A, H, rng, scale=1.0):
    """torch.nn.GRUCell's default initialisation U(-1 / sqrt(H), 1 / sqrt(H)), times `scale`."""
    k = 1.0 / np.sqrt(H)
    return ((rng.random((A, 3 * H, H)) * 2 - 1) * k * scale).astype(np.float32), ((rng.random((A, 3 * H)) * 2 - 1) * k).astype(np.float32)


class Batch(object):
    """One guarded pair of calls.  extra = (gi, save, grad): rows an episode takes beyond the minimum in gi; in h and gates; in
    dh_ext, dgi and dghn."""

    def __init__(self, B, rows, N, H, per_agent, with_hidden, with_dho, extra=(0, 0, 0), scale=1.0, seed=0):
        rng = np.random.default_rng(300 + seed)
        self.B, self.rows, self.N, self.H, self.A = B, rows, N, H, (N if per_agent else 1)
        eg, es, ex = extra
        w_hh, b_hh = draw_weights(self.A, H, rng, scale)
        host = dict(gi=rng.standard_normal((B, rows, N, 3 * H)).astype(np.float32), dh_ext=rng.standard_normal((B, rows, N, H)).astype(np.float32),
                    hidden=(rng.random((B, N, H)) * 2 - 1).astype(np.float32) if with_hidden else None,
                    d_hidden_out=rng.standard_normal((B, N, H)).astype(np.float32) if with_dho else None, w_hh=w_hh, b_hh=b_hh)
        self.host = host
        self.guards, self.whole, self.dev = {}, {}, {}
        for name, ext in (("gi", eg), ("dh_ext", ex)):           # [B, rows + ext, N, *]: NaN behind `rows`
            arr = host[name]
            self.guards[name], whole = guarded((B, rows + ext) + arr.shape[2:], torch.float32)
            whole[:, rows:] = NAN
            whole[:, :rows] = torch.from_numpy(arr).to(DEV)
            self.whole[name], self.dev[name] = whole, whole[:, :rows]
        for name in ("hidden", "d_hidden_out", "w_hh", "b_hh"):
            if host[name] is None:
                self.dev[name] = None
                continue
            self.guards[name], whole = guarded(host[name].shape, torch.float32)
            whole.copy_(torch.from_numpy(host[name]).to(DEV))
            self.whole[name] = self.dev[name] = whole
        self.used = {}
        for name, n_rows, inner in (("h", rows + es, (N, H)), ("gates", rows + es, (N, 4 * H)), ("dgi", rows + ex, (N, 3 * H)), ("dghn", rows + ex, (N, H))):
            self.guards[name], self.whole[name] = guarded((B, n_rows) + inner, torch.float32)
            self.used[name] = rows
        for name in ("hidden_out", "d_hidden_in"):
            self.guards[name], self.whole[name] = guarded((B, N, H), torch.float32)
        self.before = {k: v.clone() for k, v in self.whole.items() if k not in FWD_OUT + BWD_OUT}
        self.backward_ran = False

    def out(self, name):
        return self.whole[name][:, :self.rows] if name in self.used else self.whole[name]

    def forward(self, stream=None):
        from marbler_amd.learn import gru_scan_forward
        d = self.dev
        h, gates = gru_scan_forward(d["gi"], d["w_hh"], d["b_hh"], d["hidden"], h_out=self.out("h"), gates_out=self.out("gates"),
                                    hidden_out=self.out("hidden_out"), stream=stream)
        torch.cuda.synchronize()
        self.check_untouched(() if self.backward_ran else BWD_OUT)      # (the forward launch writes no gradient)
        assert h.data_ptr() == self.whole["h"].data_ptr() and gates.data_ptr() == self.whole["gates"].data_ptr()
        return {k: self.out(k).cpu().numpy() for k in FWD_OUT}

    def backward(self, stream=None):
        """On the h and gates the forward call left in the guarded arrays."""
        from marbler_amd.learn import gru_scan_backward
        d = self.dev
        self.before.update({k: self.whole[k].clone() for k in ("h", "gates")})
        outs = gru_scan_backward(self.out("h"), self.out("gates"), d["w_hh"], d["dh_ext"], d["hidden"], d["d_hidden_out"], dgi_out=self.out("dgi"),
                                 dghn_out=self.out("dghn"), d_hidden_in_out=self.out("d_hidden_in"), stream=stream)
        torch.cuda.synchronize()
        self.backward_ran = True
        self.check_untouched(())
        assert [o.data_ptr() for o in outs] == [self.whole[k].data_ptr() for k in BWD_OUT]
        return {k: self.out(k).cpu().numpy() for k in BWD_OUT}

    def check_untouched(self, unwritten):
        """Inputs unchanged, guard bands intact, rows behind `rows` of every output still sentinels, and so the outputs named in
        `unwritten` altogether."""
        for k, v in self.before.items():
            assert torch.equal(torch.nan_to_num(self.whole[k], nan=7.0), torch.nan_to_num(v, nan=7.0)), (k, "an input changed")
        for k, g in self.guards.items():
            assert guards_intact(g), (k, "guard band damaged")
        for k, n in self.used.items():
            assert bool((self.whole[k][:, n:] == SENTINELS[torch.float32]).all()), (k, "rows behind the last row were written")
        for k in unwritten:
            assert bool((self.whole[k] == SENTINELS[torch.float32]).all()), (k, "written by the wrong launch")

    # ------------------------------------------------------------ references
    def twin64(self):
        """Forward and backward in float64 from the inputs: h, gates, hidden_out, dgi, dghn, d_hidden_in."""
        h64 = {k: (None if v is None else v.astype(np.float64)) for k, v in self.host.items()}
        h, gates, last = tw.forward(h64["gi"], h64["w_hh"], h64["b_hh"], h64["hidden"])
        dgi, dghn, dhid = tw.backward(h, gates, h64["w_hh"], h64["dh_ext"], h64["hidden"], h64["d_hidden_out"])
        return dict(h=h, gates=gates, hidden_out=last, dgi=dgi, dghn=dghn, d_hidden_in=dhid)

    def twin64_backward_on(self, h, gates):
        """The float64 backward pass on float32 h and gates as a forward launch saved them."""
        h64 = {k: (None if v is None else v.astype(np.float64)) for k, v in self.host.items()}
        dgi, dghn, dhid = tw.backward(h.astype(np.float64), gates.astype(np.float64), h64["w_hh"], h64["dh_ext"], h64["hidden"], h64["d_hidden_out"])
        return dict(dgi=dgi, dghn=dghn, d_hidden_in=dhid)

    def torch_loop(self):
        """The torch float32 per-step loop on the device on the same inputs, and autograd through it: all six arrays."""
        d, B, N, H = self.dev, self.B, self.N, self.H
        gi = d["gi"].detach().clone().requires_grad_(True)
        hid = (d["hidden"].detach().clone() if d["hidden"] is not None else torch.zeros(B, N, H, device=DEV)).requires_grad_(True)
        w, b = d["w_hh"], d["b_hh"]
        lin = (lambda x: torch.matmul(x, w[0].t()) + b[0]) if self.A == 1 else (lambda x: torch.einsum("bnk,ngk->bng", x, w) + b)
        h, hs, gs, ghs = hid, [], [], []
        for t in range(self.rows):
            gh = lin(h)
            gh.retain_grad()
            r = torch.sigmoid(gi[:, t, :, :H] + gh[..., :H])
            z = torch.sigmoid(gi[:, t, :, H:2 * H] + gh[..., H:2 * H])
            n = torch.tanh(gi[:, t, :, 2 * H:] + r * gh[..., 2 * H:])
            h = (1.0 - z) * n + z * h
            hs.append(h), gs.append(torch.cat([r, z, n, gh[..., 2 * H:]], dim=-1)), ghs.append(gh)
        hh = torch.stack(hs, dim=1)
        loss = (hh * d["dh_ext"]).sum() + ((h * d["d_hidden_out"]).sum() if d["d_hidden_out"] is not None else 0.0)
        loss.backward()
        torch.cuda.synchronize()
        out = dict(h=hh, gates=torch.stack(gs, dim=1), hidden_out=h, dgi=gi.grad, dghn=torch.stack([g.grad[..., 2 * H:] for g in ghs], dim=1),
                   d_hidden_in=hid.grad)
        return {k: v.detach().cpu().numpy() for k, v in out.items()}


# (B, N): 1, 31, 32, 33 and 65 flat rows; with one weight set per agent (33, 2) and (13, 5) end in a ragged tile of one agent
FLAT = [(1, 1), (31, 1), (16, 2), (33, 1), (13, 5), (33, 2)]
ROWS = (1, 2, 3, 17)
EXTRA = lambda i: tuple(3 * ((i >> k) & 1) for k in range(3))     # noqa: E731  each pitch at its minimum and + 3


def _case(p, j):
    (B, N), rows = GRID[j]
    return (B, rows, N, (64, 128)[(j + j // 4 + p) % 2], bool(p), (j + j // 2 + p) % 2 == 0, (j // 2 + j // 8 + p) % 2 == 0, EXTRA(j + 3 * p + 1))


GRID = list(itertools.product(FLAT, ROWS))
# B, rows, N, H, per_agent, with_hidden, with_d_hidden_out, extra
CASES = [_case(p, j) for p in range(2) for j in range(len(GRID)) if not (p and GRID[j][0][1] == 1)]
