"""Guarded output memory for the kernel-level GPU tests (tests/test_gemm_kernels_gpu.py, tests/test_row_kernels_gpu.py)."""
import torch

DEV = "cuda"


def up(x, q):
    return (x + q - 1) // q * q


class Arena:
    """Output memory of one call: 0xFF everywhere (NaN in every float type), each tensor 16-byte aligned between two 64-byte canaries.
    spec = (name, rows, cols, dtype, ld, skew): a [rows, cols] view with row stride ld that starts `skew` elements into its region."""
    GUARD, CANARY = 64, 0xA5

    def __init__(self, specs):
        size = lambda s: (s[1] * s[4] + s[5]) * torch.empty(0, dtype=s[3]).element_size()
        total = sum(up(size(s) + 2 * self.GUARD, 16) for s in specs) + 64
        self.buf = torch.full((total,), 0xFF, dtype=torch.uint8, device=DEV)
        self.at, self.guards, self.outs, self.pads = 0, [], {}, []
        for s in specs:
            name, rows, cols, dtype, ld, skew = s
            n = size(s)
            t0 = self.at + self.GUARD
            end = t0 + n + self.GUARD
            self.buf[self.at:t0] = self.CANARY
            self.buf[t0 + n:end] = self.CANARY
            self.guards += [(self.at, t0), (t0 + n, end)]
            self.at = up(end, 16)
            raw = self.buf[t0:t0 + n].view(dtype)
            body = raw[skew:].view(rows, ld)
            self.outs[name] = body[:, :cols]
            self.pads.append((name, raw[:skew], body[:, cols:]))

    def __getitem__(self, name):
        return self.outs[name]

    def check(self, nonfinite_ok=()):
        """Canaries intact, padding untouched, every output element written and finite (but the outputs named in nonfinite_ok)."""
        for a, b in self.guards:
            assert bool((self.buf[a:b] == self.CANARY).all()), f"canary bytes {a}..{b} overwritten"
        for name, lead, pad in self.pads:
            for what, t in (("leading element", lead), ("padding columns", pad)):
                if t.numel():
                    assert bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all()), f"{name}: {what} written"
        for name, t in self.outs.items():
            if name in nonfinite_ok:
                continue
            bad = (~torch.isfinite(t.float())).nonzero()
            assert bad.numel() == 0, f"{name}: NaN / unwritten element at {bad[0].tolist()} ({bad.shape[0]} in all)"
