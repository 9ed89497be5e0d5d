"""The normal consistency loss of a triangle mesh on the GPU: ``pytorch3d.loss.mesh_normal_consistency`` for one mesh.

``sugar_trainers/refine.py:829-830`` adds ``mesh_normal_consistency(surface_mesh)`` to the loss on every iteration of the refinement, and
``SuGaR.surface_mesh`` (``sugar_model.py:524-533``) builds a fresh ``Meshes`` at every access, so nothing pytorch3d caches about the
topology survives an iteration.  pytorch3d's function hashes the ``3F`` edges and runs ``torch.unique`` over them, sorts the face-edge
incidences again, copies the per-edge counts to the host, enumerates the face pairs of every edge serially on one host core, copies the
pair table back and finishes with some fifteen torch kernels.  Here the topology becomes a *plan* in a handful of launches without a host
read (``gsr_normal_consistency_plan``), and the loss and its gradient are one fused pass each over that plan
(``gsr_normal_consistency_forward`` / ``_backward``, ``gsr_meshloss.hip``).  :func:`drop_in` is what ``autovfx_amd.install()`` puts in
place of pytorch3d's function; the ``*_host`` functions restate the contract in numpy.

The contract; the tests hold the code to this text.  Every operation is an fp32 one in the order written, nothing
contracted into a fused multiply-add; division and ``sqrt`` are the correctly rounded ones; ``max`` is C's ``fmaxf``.

An *incidence* is a (face ``f``, slot ``k``) with id ``3 f + k``.  Its edge is ``(faces[f][(k+1)%3], faces[f][(k+2)%3])`` ordered
``lo <= hi``; its opposite vertex is ``opp = faces[f][k]``.

**Plan** (``faces [F, 3]`` int64 and ``V``; topology only).  ``order [3F]`` int32: the incidence ids ascending by ``(lo, hi, id)``.
``partners [3F]`` int32: for the sorted position ``s`` the number of later positions on the same edge.  ``pairs [1]`` int64:
``P = sum(partners)``, which is the sum over the edges of ``c (c - 1) / 2`` for an edge with ``c`` incidences.  A face with any index
outside ``[0, V)`` is ignored whole: its three incidences stand at the tail of ``order``, in id order, with ``partners = 0`` (pytorch3d
would read out of bounds; difference 3).

**Forward** (``verts [V, 3]`` float32 plus the plan).  Per incidence, with ``e = v_hi - v_lo`` and ``w = v_opp - v_lo``::

    n = (e.y * w.z - e.z * w.y,  e.z * w.x - e.x * w.z,  e.x * w.y - e.y * w.x)

(pytorch3d's ``n_temp0 + n_temp1 + n_temp2``: the other two cross products are exact zeros).  A face that repeats a vertex index has
``n = 0`` exactly.  For sorted positions ``s < t`` on one edge::

    d = (n_s.x * n_t.x + n_s.y * n_t.y) + n_s.z * n_t.z
    a = max(sqrt((n_s.x^2 + n_s.y^2) + n_s.z^2), 1e-8)        b likewise of n_t
    term = 1 + d / (a * b)                                    (1 - cos(n_s, -n_t) with torch's eps)

``T_s`` is the sum of the terms of ``s``'s later partners ``t = s + 1, ..., s + partners[s]``, added in that order starting from 0.
``loss = S / float(P)``, and 0 when ``P = 0`` (pytorch3d returns ``tensor([0.])`` there, and multiplies every term by ``1 / P``;
differences 1 and 2).  ``S`` is a fixed tree over the ``T_s``, zero-padded: a halving tree (leaf ``i + 128`` onto leaf ``i``, then
``i + 64``, ...) over every 256 consecutive positions gives the partials; lane ``j`` of 1024 adds the partials ``j, j + 1024, ...`` in
chunks of 64, each chunk from 0, and the chunk sums in order from 0; a halving tree over the 1024 lanes ends it.  No ``T_s`` passes
through more than ``8 + 64 + 64 + 10 = 146`` additions (``3F < 2^30``), so with non-negative terms the relative error of ``S`` is below
``146 * 2^-24``; no float atomics: the same bits on every run.

**Backward** (plus ``grad_loss``, a device scalar) -> ``grad_verts [V, 3]``, zeroed by the call and filled with float atomics.  With
``c = grad_loss / float(P)``, per pair, ``ra`` and ``rb`` the norms before the clamp::

    q = a * b;  r = d / q
    u_s = n_t / q,  and  u_s = u_s - (r / (a * a)) * n_s   where ra > 1e-8        (the norm's derivative is off at or below the clamp)
    u_t = n_s / q,  and  u_t = u_t - (r / (b * b)) * n_t   where rb > 1e-8
    g_s = c * u_s;  g_t = c * u_t
    g_e = (w_s x g_s) + (w_t x g_t)                           (n = e x w:  d/de = w x g,  d/dw = g x e)
    the pair adds   g_e  to hi,   g_s x e  to opp_s,   g_t x e  to opp_t,   -(g_e + ((g_s x e) + (g_t x e)))  to lo

so a lane combines the ``lo`` and the ``hi`` contributions of a pair before adding: twelve atomic adds per pair.  A pair in which an
incidence repeats an index adds nothing: that incidence's own contributions cancel on the row they share, and its zero normal makes the
other side's gradient zero.  Every added term is fixed by the text above; the order of a vertex's sum is free, so the last bits of the
gradient may differ between runs (difference 4).  A vertex in no pair gets exactly 0.  At or below the clamp the norm's derivative is
off, which is autograd of ``clamp_min``; torch 2.10's ``cosine_similarity`` clamps outside autograd and lets that derivative through,
about 1 % of the gradient of a face whose normal is shorter than 1e-8 (difference 5; the loss there is pytorch3d's).

At most ``3F < 2^30`` (the radix sort's limit) and ``V < 2^31``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _takes
from ._mesh_host import cross as _cross, dot as _dot, norm as _norm, verts_faces as _verts_faces

MAX_INCIDENCES = 1 << 30
MAX_VERTS = 1 << 31
_F = np.float32
COS_EPS = _F(1e-8)
BLOCK = 256            # positions per partial
SUM_LANES = 1024       # lanes of the second stage
SUM_CHUNK = 64         # partials a lane adds before the chunk sums are added


class NormalConsistencyPlan(NamedTuple):
    """What :func:`plan` makes of a topology: ``order [3F]`` int32, ``partners [3F]`` int32, ``pairs [1]`` int64, on the faces' device."""
    order: torch.Tensor
    partners: torch.Tensor
    pairs: torch.Tensor


# ---- which calls the kernels take -----------------------------------------------------------------------------------------------------

HOST = "mesh_normal_consistency_host"
ALLOCATES = "the call allocates its scratch; such a call is left to the original"


def _why_not(verts, faces, plan_=None, needs_faces: bool = False) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    why = _takes.mesh(verts, faces, HOST) or _why_not_counts(faces.shape[0], verts.shape[0])
    if why is not None:
        return why
    if needs_faces and faces.shape[0] < 1:
        return "a mesh without faces"
    if plan_ is not None:
        n = 3 * faces.shape[0]
        for name, t, dtype, count in (("order", plan_.order, torch.int32, n), ("partners", plan_.partners, torch.int32, n),
                                      ("pairs", plan_.pairs, torch.int64, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != faces.device or tuple(t.shape) != (count,) \
                    or not t.is_contiguous():
                return f"plan.{name} must be a contiguous {dtype} [{count}] on {faces.device}: the plan of these faces"
    return _takes.capturing(ALLOCATES)


def _why_not_faces(faces, V) -> Optional[str]:
    """As :func:`_why_not`, for the faces alone and a ``V`` the caller states."""
    return (_takes.tensors((("faces", faces, torch.int64),), host=HOST)
            or _takes.shaped("faces", faces, "[F, 3]", faces.dim() == 2 and faces.shape[1] == 3) or _why_not_counts(faces.shape[0], V))


def _why_not_counts(F, V) -> Optional[str]:
    if type(V) is not int or V < 0:
        return f"V must be a non-negative int (got {V!r})"
    if 3 * F >= MAX_INCIDENCES or V >= MAX_VERTS:
        return f"{F} faces, {V} vertices: 3 F below 2^30 and V below 2^31"
    return None


# ---- the calls ------------------------------------------------------------------------------------------------------------------------

def _plan(faces: torch.Tensor, V: int) -> NormalConsistencyPlan:
    from . import _lib

    f = _takes.c(faces)
    F = int(f.shape[0])
    order = torch.empty((3 * F,), dtype=torch.int32, device=f.device)
    partners = torch.empty((3 * F,), dtype=torch.int32, device=f.device)
    pairs = torch.empty((1,), dtype=torch.int64, device=f.device)
    with torch.cuda.device(f.device):
        scratch, nbytes = _lib.scratch("gsr_normal_consistency_plan_scratch_bytes", F, device=f.device)
        _lib.call("gsr_normal_consistency_plan", V, F, _lib.ptr(f), _lib.ptr(order), _lib.ptr(partners), _lib.ptr(pairs), _lib.ptr(scratch),
                  nbytes, device=f.device)
    return NormalConsistencyPlan(order, partners, pairs)


def _forward(v: torch.Tensor, f: torch.Tensor, p: NormalConsistencyPlan, want_terms: bool = False):
    """Contiguous ``v``, ``f`` and a checked plan -> ``(loss, terms or None)``."""
    from . import _lib

    V, F = int(v.shape[0]), int(f.shape[0])
    loss = torch.empty((), dtype=torch.float32, device=v.device)
    terms = torch.empty((3 * F,), dtype=torch.float32, device=v.device) if want_terms else None
    with torch.cuda.device(v.device):
        scratch, nbytes = _lib.scratch("gsr_normal_consistency_scratch_bytes", F, device=v.device)
        _lib.call("gsr_normal_consistency_forward", V, F, _lib.ptr(v), _lib.ptr(f), _lib.ptr(p.order), _lib.ptr(p.partners), _lib.ptr(p.pairs),
                  _lib.ptr(loss), _lib.ptr(terms), _lib.ptr(scratch), nbytes, device=v.device)
    return loss, terms


def _backward(v: torch.Tensor, f: torch.Tensor, p: NormalConsistencyPlan, grad_loss: torch.Tensor) -> torch.Tensor:
    from . import _lib

    V, F = int(v.shape[0]), int(f.shape[0])
    g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
    grad_verts = torch.empty((V, 3), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.call("gsr_normal_consistency_backward", V, F, _lib.ptr(v), _lib.ptr(f), _lib.ptr(p.order), _lib.ptr(p.partners), _lib.ptr(p.pairs),
                  _lib.ptr(g), _lib.ptr(grad_verts), device=v.device)
    return grad_verts


class _NormalConsistency(torch.autograd.Function):
    """Forward and backward are the kernels; differentiable once, in ``verts``."""

    @staticmethod
    def forward(ctx, verts, faces, order, partners, pairs):
        v, f = _takes.cs(verts, faces)
        p = NormalConsistencyPlan(order, partners, pairs)
        loss, _ = _forward(v, f, p)
        ctx.save_for_backward(v, f, order, partners, pairs)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        v, f, order, partners, pairs = ctx.saved_tensors
        return _backward(v, f, NormalConsistencyPlan(order, partners, pairs), grad_loss), None, None, None, None


def plan(faces, V: int) -> NormalConsistencyPlan:
    """The plan of a topology (the module's contract), queued on the current stream without a host read.  A caller whose faces do not
    change builds it once and passes it to :func:`mesh_normal_consistency`; the faces it is used with must be the ones it was built from."""
    _takes.refuse("plan", _why_not_faces(faces, V) or _takes.capturing(ALLOCATES))
    return _plan(faces, V)


def mesh_normal_consistency(verts, faces, plan: Optional[NormalConsistencyPlan] = None) -> torch.Tensor:
    """The loss of the module's contract for ``verts [V, 3]`` float32 and ``faces [F, 3]`` int64 on one GPU: a 0-dim tensor, differentiable
    once in ``verts``, queued on the current stream with no host synchronisation.  ``plan``: what :func:`plan` returned for these faces and
    this ``V`` (the two sorts are then skipped); built per call when not given.  Non-contiguous inputs are copied.  ``F = 0`` gives 0.
    A call the kernels do not take raises ``ValueError`` with the reason."""
    _takes.refuse("mesh_normal_consistency", _why_not(verts, faces, plan))
    p = plan if plan is not None else _plan(faces, int(verts.shape[0]))
    return _NormalConsistency.apply(verts, faces, p.order, p.partners, p.pairs)


def mesh_normal_consistency_terms(verts, faces, plan: Optional[NormalConsistencyPlan] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss, terms [3F])`` without autograd: the ``T_s`` of the contract beside the loss (for tests and diagnosis)."""
    _takes.refuse("mesh_normal_consistency_terms", _why_not(verts, faces, plan))
    p = plan if plan is not None else _plan(faces, int(verts.shape[0]))
    return _forward(*_takes.cs(verts, faces), p, want_terms=True)


def _packed(meshes):
    """``(verts, faces)`` of a one-mesh ``Meshes`` the kernels take, else None."""
    try:
        if len(meshes) != 1:
            return None
        verts, faces = meshes.verts_packed(), meshes.faces_packed()
    except (AttributeError, TypeError):
        return None
    return (verts, faces) if _why_not(verts, faces, needs_faces=True) is None else None


def drop_in(original: Callable) -> Callable:
    """A ``mesh_normal_consistency(meshes)`` that runs the kernels when ``len(meshes) == 1``, ``verts_packed()`` is CUDA float32 ``[V, 3]``,
    ``faces_packed()`` int64 ``[F, 3]`` on the same device with ``F >= 1`` and no graph is being captured, and ``original`` (pytorch3d's)
    with the caller's arguments for every other call: batches, CPU meshes, an empty mesh, other dtypes, objects without those methods.
    The plan is built on every call: ``Meshes.__init__`` re-indexes the faces, so a tensor's identity proves nothing about the topology,
    and checking the content would need the host round trip this replaces."""
    def mesh_normal_consistency_drop_in(*args, **kwargs):
        taken = _packed(args[0]) if len(args) == 1 and not kwargs else None
        if taken is None:
            return original(*args, **kwargs)
        verts, faces = taken
        p = _plan(faces, int(verts.shape[0]))
        return _NormalConsistency.apply(verts, faces, p.order, p.partners, p.pairs)

    return _takes.dressed(mesh_normal_consistency_drop_in, "mesh_normal_consistency", original, "pytorch3d.loss.mesh_normal_consistency", "meshloss")


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------

def _incidences(faces: np.ndarray, V: int, ids: np.ndarray):
    """``valid, lo, hi, opp`` of the incidences ``ids`` (an id outside ``[0, 3F)`` is not valid; ``lo = hi = V`` where not valid)."""
    n = 3 * faces.shape[0]
    inside = (ids >= 0) & (ids < n)
    safe = np.where(inside, ids, 0)
    f, k = safe // 3, safe % 3
    if n == 0:
        none = np.full(ids.shape, V, np.int64)
        return np.zeros(ids.shape, bool), none, none.copy(), none.copy()
    rows = faces[f]
    valid = inside & ((rows >= 0) & (rows < V)).all(axis=1)
    at = np.arange(len(ids))
    opp, a, b = rows[at, k], rows[at, (k + 1) % 3], rows[at, (k + 2) % 3]
    lo, hi = np.where(valid, np.minimum(a, b), V), np.where(valid, np.maximum(a, b), V)
    return valid, lo, hi, np.where(valid, opp, V)


def plan_host(faces, V: int):
    """The plan of the module's contract in numpy, by the kernels' route: two stable sorts, by ``hi`` and then by ``lo``, and the run
    lengths of the sorted edges.  Returns ``(order [3F] int32, partners [3F] int32, pairs int)``."""
    faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    n = 3 * faces.shape[0]
    _valid, lo, hi, _opp = _incidences(faces, V, np.arange(n, dtype=np.int64))
    order = np.argsort(hi, kind="stable")
    order = order[np.argsort(lo[order], kind="stable")]
    lo_s, hi_s = lo[order], hi[order]
    partners = np.zeros(n, np.int64)
    if n:
        first = np.concatenate(([True], (lo_s[1:] != lo_s[:-1]) | (hi_s[1:] != hi_s[:-1])))
        starts = np.nonzero(first)[0]
        ends = np.concatenate((starts[1:], [n]))
        partners = ends[np.cumsum(first) - 1] - 1 - np.arange(n)
        partners[lo_s == V] = 0
    return order.astype(np.int32), partners.astype(np.int32), int(partners.sum())


class _Walks(NamedTuple):
    valid: np.ndarray      # [3F] the position's face has its indices in range
    lo: np.ndarray
    hi: np.ndarray
    opp: np.ndarray
    e: np.ndarray          # [3F, 3] zeros where not valid
    w: np.ndarray
    n: np.ndarray
    count: np.ndarray      # [3F] partners a lane walks: none for a position that is not valid, never past the end


def _walks(verts: np.ndarray, faces: np.ndarray, order: np.ndarray, partners: np.ndarray) -> _Walks:
    n, V = 3 * faces.shape[0], verts.shape[0]
    valid, lo, hi, opp = _incidences(faces, V, np.asarray(order, np.int64))
    e, w = np.zeros((n, 3), _F), np.zeros((n, 3), _F)
    with np.errstate(all="ignore"):
        if valid.any():
            v_lo = verts[lo[valid]]
            e[valid], w[valid] = verts[hi[valid]] - v_lo, verts[opp[valid]] - v_lo
        normal = _cross(e, w).astype(_F)
    count = np.clip(np.asarray(partners, np.int64), 0, np.maximum(n - 1 - np.arange(n), 0))
    return _Walks(valid, lo, hi, opp, e, w, normal, np.where(valid, count, 0))


def _pairs_of(k: _Walks):
    """``(s, t)`` of every pair the lanes visit, partner distance by partner distance: ``s`` ascending within one distance."""
    ss, tt = [], []
    for j in range(1, int(k.count.max()) + 1 if len(k.count) else 1):
        s = np.nonzero(k.count >= j)[0]
        s = s[k.valid[s + j]]
        ss.append(s), tt.append(s + j)
    if not ss:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ss), np.concatenate(tt)


def tree_sum_host(terms) -> np.float32:
    """``S`` of the module's contract: the fixed tree over the ``T_s``."""
    terms = np.asarray(terms, _F).reshape(-1)
    if terms.size == 0:
        return _F(0.0)

    def halving(x):                                   # [rows, 2^m] -> [rows]
        while x.shape[1] > 1:
            half = x.shape[1] // 2
            x = x[:, :half] + x[:, half:]
        return x[:, 0]

    with np.errstate(all="ignore"):
        padded = np.zeros(-(-terms.size // BLOCK) * BLOCK, _F)
        padded[:terms.size] = terms
        partials = halving(padded.reshape(-1, BLOCK))
        span = SUM_LANES * SUM_CHUNK
        padded = np.zeros(-(-partials.size // span) * span, _F)
        padded[:partials.size] = partials
        chunks = padded.reshape(-1, SUM_CHUNK, SUM_LANES)          # [chunk, item, lane]: partial lane + 1024 (64 chunk + item)
        lanes = np.zeros(SUM_LANES, _F)
        for q in range(chunks.shape[0]):
            chunk = np.zeros(SUM_LANES, _F)
            for r in range(SUM_CHUNK):
                chunk = chunk + chunks[q, r]
            lanes = lanes + chunk
        return _F(halving(lanes.reshape(1, -1))[0])


def mesh_normal_consistency_host(verts, faces, plan=None):
    """The forward of the module's contract in numpy, every operation an fp32 elementwise one in the contract's order.  ``plan``: what
    :func:`plan_host` returns (built when None).  Returns ``(loss, terms [3F])``, float32."""
    verts, faces = _verts_faces(verts, faces)
    order, partners, P = plan if plan is not None else plan_host(faces, verts.shape[0])
    k = _walks(verts, faces, order, partners)
    terms = np.zeros(len(order), _F)
    with np.errstate(all="ignore"):
        a = np.fmax(_norm(k.n), COS_EPS)
        s_all, t_all = _pairs_of(k)
        # (one partner distance at a time: a position's terms are added in ascending order of t)
        for j in np.unique(t_all - s_all):
            at = (t_all - s_all) == j
            s, t = s_all[at], t_all[at]
            terms[s] = terms[s] + (_F(1.0) + _dot(k.n[s], k.n[t]) / (a[s] * a[t]))
        S = tree_sum_host(terms)
        loss = S / _F(P) if P > 0 else _F(0.0)
    return _F(loss), terms


def mesh_normal_consistency_backward_host(verts, faces, grad_loss, plan=None):
    """The backward of the module's contract in numpy.  Returns ``(grad_verts [V, 3], terms [T, 3], rows [T])``: the fp32 terms the kernel
    adds and the vertex each goes to (four per pair: hi, lo, opp_s, opp_t), each fixed by the contract; ``grad_verts`` is their fp32 sum in
    that order, one of the orders the kernel's atomics may take."""
    verts, faces = _verts_faces(verts, faces)
    order, partners, P = plan if plan is not None else plan_host(faces, verts.shape[0])
    k = _walks(verts, faces, order, partners)
    grad_verts = np.zeros(verts.shape, _F)
    s, t = _pairs_of(k)
    repeats = (k.lo == k.hi) | (k.opp == k.lo) | (k.opp == k.hi)
    keep = ~(repeats[s] | repeats[t])
    s, t = s[keep], t[keep]
    if P <= 0 or len(s) == 0:
        return grad_verts, np.zeros((0, 3), _F), np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        c = _F(grad_loss) / _F(P)
        ns, nt, e, ws, wt = k.n[s], k.n[t], k.e[s], k.w[s], k.w[t]
        ra, rb = _norm(ns), _norm(nt)
        a, b = np.fmax(ra, COS_EPS), np.fmax(rb, COS_EPS)
        q = a * b
        r = _dot(ns, nt) / q
        us = nt / q[:, None]
        us = np.where((ra > COS_EPS)[:, None], us - (r / (a * a))[:, None] * ns, us)
        ut = ns / q[:, None]
        ut = np.where((rb > COS_EPS)[:, None], ut - (r / (b * b))[:, None] * nt, ut)
        gs, gt = c * us, c * ut
        g_e = _cross(ws, gs) + _cross(wt, gt)
        g_ws, g_wt = _cross(gs, e), _cross(gt, e)
        g_lo = -(g_e + (g_ws + g_wt))
        terms = np.concatenate((g_e, g_lo, g_ws, g_wt)).astype(_F)
        rows = np.concatenate((k.hi[s], k.lo[s], k.opp[s], k.opp[t])).astype(np.int64)
        np.add.at(grad_verts, rows, terms)
    return grad_verts, terms, rows
