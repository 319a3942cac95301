"""Pair scoring (include/gnnagg.h section G): one value -- or one row of n_out values -- per node pair in ONE launch
(csrc/agg_pair_score.hip): the dot-product and DistMult decoders and the Hadamard / concat two-layer MLP of link predictors and edge
classifiers, over COO pairs or the positions of a CSR.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib
from .aggregator import FEATURE_DTYPES, _dev_ptr, _dev_ptr_rows, _feat_dtype, matmul_NN

KINDS = {"dot": _lib.PAIR_DOT, "mlp": _lib.PAIR_MLP}
COMBINES = {"mul": _lib.PAIR_MUL, "cat": _lib.PAIR_CAT}


def pair_score_supported(kind, combine, feat, hidden, n_out, dtype):
    """gnnagg_pair_score_supported: does the kernel serve this kind ("dot" / "mlp"), combine ("mul" / "cat"), shape and operand dtype?"""
    return (kind in KINDS and combine in COMBINES and dtype in FEATURE_DTYPES
            and bool(lib().gnnagg_pair_score_supported(KINDS[kind], COMBINES[combine], int(feat), int(hidden), int(n_out), FEATURE_DTYPES[dtype])))


def pair_score_prefers_fused(num_pairs, combine, feat, hidden, n_out, dtype):
    """The fused=None rule of pair_score(kind="mlp"): the kernel wherever it is supported.  (profiles/pair_score/README.md: the shapes
    measured and what each arm took.)"""
    return pair_score_supported("mlp", combine, feat, hidden, n_out, dtype)


def pair_score(hu, hv, u=None, v=None, ptr=None, idx=None, src=None, kind="dot", rel=None, etype=None, combine="mul", w1=None, w2=None, b1=None,
               b2=None, relu=False, out=None, out_dtype=None, fused=None):
    """Scores P node pairs (u_p, v_p) in ONE launch on torch's current stream (gnnagg_pair_score_run).
      hu, hv       float32 or bfloat16 [rows, F], one dtype; row-pitched column views (stride(1) == 1) are taken as they are; may be one tensor
      u, v         int32 [P]: the pairs as COO -- or --
      ptr, idx     int32 [n + 1], [P]: the pairs as the positions of a CSR, u_p = the row that owns position p (found by the kernel), v_p = idx[p]
      src          None or int32: the row map of a relabelled block, applied to both ids (hu row = src[u_p], hv row = src[v_p])
      kind="dot"   out[p] = sum_f hu[u_p, f] * hv[v_p, f], float32 [P].  With rel (float32 [R, F]) and etype (int32 [P]) DistMult:
                   out[p] = sum_f hu[u_p, f] * rel[t_p, f] * hv[v_p, f]; a pair whose type lies outside [0, R) scores +0.
      kind="mlp"   out[p] = act(relu(m_p @ w1 + b1) @ w2 + b2), [P, n_out]; combine="mul": m_p = hu[u_p] * hv[v_p], w1 [F, H];
                   combine="cat": m_p = cat(hu[u_p], hv[v_p]), w1 [2 F, H].  w2 [H, n_out]; both of hu's dtype; b1, b2 float32 or None;
                   relu: the activation of out (the hidden ReLU is always applied).  out: float32 for float32 operands, float32 or
                   bfloat16 for bfloat16 operands (out_dtype; hu's by default).
      fused        kind="mlp" only.  True: the kernel, ValueError where pair_score_supported says no.  False: the composition of existing
                   calls (the index of both row sets, * or cat, matmul_NN, bias, ReLU, matmul_NN, bias, ReLU) -- for float32 the same
                   bits.  None: the kernel where it is supported and was not measured slower (pair_score_prefers_fused).
    Every dtype and shape refusal is raised before device work.  Returns out."""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
    if combine not in COMBINES:
        raise ValueError("combine must be one of %s, got %r" % (sorted(COMBINES), combine))
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    dot = kind == "dot"
    # the pairs
    coo, csr = u is not None or v is not None, ptr is not None or idx is not None
    if coo == csr:
        raise ValueError("the pairs come as (u, v) or as (ptr, idx): %s were given" % ("both" if coo else "neither"))
    for name, t in (("u", u), ("v", v)) if coo else (("ptr", ptr), ("idx", idx)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
            raise TypeError("%s must be a 1-D torch.int32 tensor, got %s" % (name, getattr(t, "dtype", type(t).__name__)))
    if coo and u.numel() != v.numel():
        raise ValueError("u and v must have one length, got %d and %d" % (u.numel(), v.numel()))
    if csr and ptr.numel() < 2:
        raise ValueError("ptr must hold n + 1 >= 2 entries, got %d" % ptr.numel())
    num_pairs, num_rows = int((v if coo else idx).numel()), (0 if coo else int(ptr.numel()) - 1)
    if src is not None and (not isinstance(src, torch.Tensor) or src.dtype != torch.int32 or src.dim() != 1):
        raise TypeError("src must be a 1-D torch.int32 tensor or None")
    # types and shapes
    xdt = _feat_dtype(hu, "hu")
    if not isinstance(hv, torch.Tensor) or hv.dtype != hu.dtype:
        raise TypeError("hv must be a tensor of hu's dtype %s, got %s" % (hu.dtype, getattr(hv, "dtype", type(hv).__name__)))
    if hu.dim() != 2 or hu.shape[1] < 1:
        raise ValueError("hu must be 2-D [rows, F] with F >= 1, got %s" % (tuple(hu.shape),))
    feat = int(hu.shape[1])
    if hv.dim() != 2 or int(hv.shape[1]) != feat:
        raise ValueError("hv must be [rows, %d] as hu, got %s" % (feat, tuple(hv.shape)))
    if (rel is None) != (etype is None):
        raise ValueError("rel and etype come together (DistMult): %s is missing" % ("etype" if etype is None else "rel"))
    hidden = n_out = num_rel = 0
    if dot:
        for name, t in (("w1", w1), ("w2", w2), ("b1", b1), ("b2", b2)):
            if t is not None:
                raise ValueError("%s is given: kind=\"dot\" takes no weights" % name)
        if relu or combine != "mul" or fused is not None:
            raise ValueError("relu, combine and fused belong to kind=\"mlp\"")
        if rel is not None:
            if not isinstance(rel, torch.Tensor) or rel.dtype != torch.float32:
                raise TypeError("rel must be a torch.float32 tensor")
            if rel.dim() != 2 or int(rel.shape[0]) < 1 or int(rel.shape[1]) != feat:
                raise ValueError("rel must be [R, %d] with R >= 1, got %s" % (feat, tuple(rel.shape)))
            if not isinstance(etype, torch.Tensor) or etype.dtype != torch.int32:
                raise TypeError("etype must be a torch.int32 tensor")
            if tuple(etype.shape) != (num_pairs,):
                raise ValueError("etype must be [%d], one type per pair, got %s" % (num_pairs, tuple(etype.shape)))
            num_rel = int(rel.shape[0])
        shape = (num_pairs,)
    else:
        if rel is not None:
            raise ValueError("rel and etype belong to kind=\"dot\"")
        for name, w in (("w1", w1), ("w2", w2)):
            if not isinstance(w, torch.Tensor) or w.dtype != hu.dtype:
                raise TypeError("%s must be a tensor of hu's dtype %s, got %s" % (name, hu.dtype, getattr(w, "dtype", type(w).__name__)))
        k1 = 2 * feat if combine == "cat" else feat
        if w1.dim() != 2 or int(w1.shape[0]) != k1 or int(w1.shape[1]) < 1:
            raise ValueError("w1 must be [%d, hidden] with hidden >= 1 (combine=%r), got %s" % (k1, combine, tuple(w1.shape)))
        hidden = int(w1.shape[1])
        if w2.dim() != 2 or int(w2.shape[0]) != hidden or int(w2.shape[1]) < 1:
            raise ValueError("w2 must be [%d, n_out] with n_out >= 1, got %s" % (hidden, tuple(w2.shape)))
        n_out = int(w2.shape[1])
        for name, b, n in (("b1", b1, hidden), ("b2", b2, n_out)):
            if b is None:
                continue
            if not isinstance(b, torch.Tensor) or b.dtype != torch.float32:
                raise TypeError("%s must be a torch.float32 tensor or None" % name)
            if tuple(b.shape) != (n,):
                raise ValueError("%s must be [%d], got %s" % (name, n, tuple(b.shape)))
        shape = (num_pairs, n_out)
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be %s, got %s" % (list(shape), tuple(out.shape)))
    odt = out.dtype if out is not None else (out_dtype or (torch.float32 if dot else hu.dtype))
    if odt != torch.float32 and (dot or hu.dtype == torch.float32):
        raise TypeError("out_dtype: %s give a float32 out, got %s" % ("kind=\"dot\" scores" if dot else "float32 operands", odt))
    if fused and not pair_score_supported(kind, combine, feat, hidden, n_out, hu.dtype):
        raise ValueError("fused=True: gnnagg_pair_score_supported(%s, %s, feat=%d, hidden=%d, n_out=%d, %s) says no"
                         % (kind, combine, feat, hidden, n_out, hu.dtype))
    # device tensors, contiguous where the call wants them dense
    p_hu, upitch = _dev_ptr_rows(hu, hu.dtype, "hu")
    p_hv, vpitch = _dev_ptr_rows(hv, hu.dtype, "hv")
    p_u, p_v = _dev_ptr(u, torch.int32, "u"), _dev_ptr(v, torch.int32, "v")
    p_ptr, p_idx, p_src = _dev_ptr(ptr, torch.int32, "ptr"), _dev_ptr(idx, torch.int32, "idx"), _dev_ptr(src, torch.int32, "src")
    p_rel, p_et = _dev_ptr(rel, torch.float32, "rel"), _dev_ptr(etype, torch.int32, "etype")
    p_w1, p_w2 = _dev_ptr(w1, hu.dtype, "w1"), _dev_ptr(w2, hu.dtype, "w2")
    p_b1, p_b2 = _dev_ptr(b1, torch.float32, "b1"), _dev_ptr(b2, torch.float32, "b2")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("hv", hv), ("u", u), ("v", v), ("ptr", ptr), ("idx", idx), ("src", src), ("rel", rel), ("etype", etype), ("w1", w1),
                    ("w2", w2), ("b1", b1), ("b2", b2), ("out", out)):
        if t is not None and t.device != hu.device:
            raise ValueError("%s lives on %s, hu on %s" % (name, t.device, hu.device))
    # ---- device work
    if not dot and fused is None:
        fused = pair_score_prefers_fused(num_pairs, combine, feat, hidden, n_out, hu.dtype)
    if not dot and not fused:   # the composition a caller writes with the existing calls
        if csr:
            u = torch.searchsorted(ptr[1:].long().contiguous(), torch.arange(num_pairs, device=hu.device), right=True)
            v = idx
        ru, rv = (src[u.long()].long(), src[v.long()].long()) if src is not None else (u.long(), v.long())
        m = torch.cat([hu[ru], hv[rv]], 1) if combine == "cat" else hu[ru] * hv[rv]
        z = matmul_NN(m, w1, out_dtype=torch.float32)
        if b1 is not None:
            z = z + b1
        z = z.clamp_min(0).to(hu.dtype)
        res = matmul_NN(z, w2, out_dtype=torch.float32)
        if b2 is not None:
            res = res + b2
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=hu.device)
    has = num_pairs > 0
    check(lib().gnnagg_pair_score_run(KINDS[kind], COMBINES[combine], p_u if has else None, p_v if has else None, p_ptr if has else None,
                                      p_idx if has else None, num_rows, num_pairs, p_src, p_hu, upitch, p_hv, vpitch, xdt, feat, p_rel, p_et,
                                      num_rel, p_w1, p_b1, hidden, p_w2, p_b2, n_out, ctypes.c_void_p(out.data_ptr()) if has else None,
                                      FEATURE_DTYPES[out.dtype], _lib.FLAG_RELU if relu else 0,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out
