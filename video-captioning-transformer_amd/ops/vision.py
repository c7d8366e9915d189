"""The vision tower's own kernels (csrc/vct_vision.hip): frame preprocessing into patch rows, the class / position / ln_pre assembly
and the class-row pool."""
import torch

from .. import _lib as L


def frames_to_patches(frames, tables, lut, P, out, crop=None):
    """frames uint8 [N, H, W, 3] contiguous -> out [N * G * G, 3 * P * P] (dtype of `lut`), G = R / P: PIL's bicubic resize, centre
    crop and the per-channel value table, per patch row (include/vct_hip.h, vct_frames_to_patches).
    tables: dict(R, hx_min, hx_len, hx_w [R, kx], vy_min, vy_len, vy_w [R, ky] int32 on the device, stage_rows[P] on the host), as
    vision.device_tables builds them for this (H, W); lut [3, 256]; crop: uint8 [N, R, R, 3] or None."""
    N, H, W, _ = frames.shape
    R = tables["R"]
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
    assert P >= 1 and R % P == 0 and lut.dtype == out.dtype and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
    G = R // P
    assert out.is_contiguous() and tuple(out.shape) == (N * G * G, 3 * P * P)
    assert crop is None or (crop.dtype == torch.uint8 and crop.is_contiguous() and tuple(crop.shape) == (N, R, R, 3))
    t = tables
    for k in ("hx_min", "hx_len", "vy_min", "vy_len"):
        assert t[k].dtype == torch.int32 and t[k].numel() == R and t[k].is_contiguous()
    for k in ("hx_w", "vy_w"):
        assert t[k].dtype == torch.int32 and t[k].dim() == 2 and t[k].shape[0] == R and t[k].is_contiguous()
    L.check(L.load().vct_frames_to_patches(L.dtype_code(out.dtype), N, H, W, R, P, frames.data_ptr(), t["hx_min"].data_ptr(),
                                           t["hx_len"].data_ptr(), t["hx_w"].data_ptr(), t["hx_w"].shape[1], t["vy_min"].data_ptr(),
                                           t["vy_len"].data_ptr(), t["vy_w"].data_ptr(), t["vy_w"].shape[1], int(t["stage_rows"][P]),
                                           lut.data_ptr(), out.data_ptr(), L.ptr(crop), L.stream_ptr()), "vct_frames_to_patches")
    return out


def vit_embed(e, cls, pos, gamma, beta, x):
    """x[n * L + l] = LayerNorm(l == 0 ? cls + pos[0] : e[n * (L - 1) + l - 1] + pos[l]): e fp32 [N * (L - 1), d], pos fp32 [L, d],
    x fp32 [N * L, d] (include/vct_hip.h, vct_vit_embed)."""
    Lr, dm = pos.shape
    assert Lr >= 2 and e.dim() == 2 and e.shape[0] % (Lr - 1) == 0 and e.shape[1] == dm
    N = e.shape[0] // (Lr - 1)
    for t in (e, cls, pos, gamma, beta, x):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert cls.numel() == gamma.numel() == beta.numel() == dm and tuple(x.shape) == (N * Lr, dm)
    L.check(L.load().vct_vit_embed(N, Lr, dm, e.data_ptr(), cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                   x.data_ptr(), L.stream_ptr()), "vct_vit_embed")
    return x


def vit_pool(x, S, gamma, beta, y):
    """y[n] = LayerNorm(x[n * S]): the class rows of the fp32 stream x [N * S, d]; y [N, d] fp32 or bf16 (include/vct_hip.h,
    vct_vit_pool)."""
    N, dm = y.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (N * S, dm) and y.is_contiguous()
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == dm
    L.check(L.load().vct_vit_pool(L.dtype_code(y.dtype), N, S, dm, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                  L.stream_ptr()), "vct_vit_pool")
    return y
