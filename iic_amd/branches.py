"""Two-stream execution state: which branch the calling code is on, the side streams, the per-branch leaf aliases
of the parameters, the forks not joined yet and the running-statistic updates they postponed.  One BranchContext
per thread owns all of it; `context()` returns it and every user works on its fields.
"""
import ctypes
import os
import threading
import weakref

import torch

from ._lib import check, lib, ptr, stream_ptr


# ------------------------------------------------------------------------------------
# Branches: two independent forwards of a step (net(all_imgs), net(all_imgs_tf):
# cluster_sobel.py:238-239) can run on two HIP streams -- as two parallel branches of the captured
# step graph -- so that the tail of one view's kernel is filled by the other view's next kernel
# (measured: 42.6 -> 38.2 ms for the two forward+backward passes, tools/graph_probes.py dual_branch_probe).
# Everything the kernels share through HBM is therefore keyed by the branch index: PT buffers,
# BatchNorm statistic accumulators, split-K / stem scratch, the bf16 weight operands.  A branch's
# autograd Functions remember their branch (ctx.branch) and restore it in backward, where the
# engine already runs them on the stream they were recorded on.
#   with ops.branch():            # fork: side stream waits for the current one
#     xo = net(all_imgs)          # the view that comes FIRST is enqueued on the side stream
#   xt = net(all_imgs_tf)         # main stream, concurrently
#   ops.join()                    # the current stream waits for the side stream (the losses and
#                                 # the optimiser call it themselves if it is still pending)
# Inside a branch: parameters are seen through per-branch leaf aliases (`pv`), so that gradient
# accumulation of shared parameters never synchronises the branches (the optimiser adds the two
# gradient sets, iic_amd.optim.Adam); while a branch is pending, BatchNorm running-statistic
# updates of BOTH views are postponed to the join and applied there in call order -- the order a
# sequential run would have used (ops.bn_finalize -> BranchContext.deferred_running).
# ------------------------------------------------------------------------------------
class BranchContext(object):
  """Everything the two-stream execution keeps between calls, in ONE object per thread (round 6; until round 5 these
  were nine module-level lists / dicts, which is the style that produced round 5's read-before-join race): the branch
  the calling code is on, the side streams, the per-branch leaf aliases of the parameters, the forks not joined yet
  and the running-statistic updates they postponed.  One process drives one device (the data-parallel design: one
  process per GPU), so a context is per thread, and its streams are keyed by device inside.  The autograd engine runs
  backward nodes on its own threads: every Function records its branch at forward time (ctx.branch) and
  `branch_backward` restores it there, so a backward thread never depends on the forward thread's context."""
  __slots__ = ("branch", "streams", "proxies", "deferred_running", "pending_join", "branch_main", "no_proxy_branches",
               "capture_proxies", "solo_first")

  def __init__(self):
    self.branch = 0                 # 0 = the caller's stream, >= 1 = a side branch / resource namespace
    self.streams = {}               # (device, branch index) -> side stream
    self.proxies = {}               # id(param) -> (param, {branch: leaf alias sharing its storage})
    self.deferred_running = []      # (coef, running_mean, running_var, num_batches_tracked, C) of a branch forward
    self.pending_join = []          # (main stream, side stream) of branches not joined yet
    # inside `with branch():` the stream the caller was on (iic_amd.graphed orders it after a view's backward)
    self.branch_main = None
    # Branch indices that see the parameters themselves (no leaf aliases): the side stream of auto_branch -- only
    # captured / replayed views run there, and those hand their gradients over explicitly (iic_amd/graphed.py) -- and
    # the resource namespaces iic_amd.graphed gives to positions that share a real branch.
    # (Rounds 3-4 also had an EAGER two-stream mode for unchanged scripts -- leaf aliases plus an end-of-backward fold
    # of the alias gradients into .grad.  It was demoted to opt-in in round 4 because about 1 run in 13 differed from
    # the one-stream run; round 5 found the cause -- the loss stacked the forked view's outputs before joining it,
    # iic_amd/losses.py -- and removed the mode rather than carry a second gradient hand-over for launches that are
    # host-bound anyway.)
    self.no_proxy_branches = set()
    self.capture_proxies = None     # iic_amd.graphed: {id(param): leaf alias} while a view's graphs are captured
    # 1: the first forward of an auto_branch pair ran EAGERLY on the caller's stream, so the second one must not fork
    # either; both views' running-statistic updates are postponed and the second forward's join clears it
    self.solo_first = 0

  def as_branch(self, index):
    """`with ctx.as_branch(index):` -- the enclosed code runs as branch / resource namespace `index` (no stream
    change, no fork or join), and the previous branch comes back afterwards."""
    return _AsBranch(self, index)


class _AsBranch(object):
  __slots__ = ("ctx", "index", "prev")

  def __init__(self, ctx, index):
    self.ctx, self.index = ctx, index

  def __enter__(self):
    self.prev = self.ctx.branch
    self.ctx.branch = self.index

  def __exit__(self, *exc):
    self.ctx.branch = self.prev
    return False


_TLS = threading.local()


def context():
  """The calling thread's BranchContext."""
  c = getattr(_TLS, "ctx", None)
  if c is None:
    c = _TLS.ctx = BranchContext()
  return c


def current_branch():
  """The branch index the calling thread is on (pool keys, statistic keys, ctx.branch of the autograd Functions)."""
  return context().branch


# IIC_BRANCH_PROXIES=0 (debugging only): side branches use the parameters themselves and autograd accumulates both
# views' gradients into p.grad ACROSS the two streams.
USE_PROXIES = [os.environ.get("IIC_BRANCH_PROXIES", "1") != "0"]


def pv(p):
  """Parameter as seen by the current branch (the parameter itself on the main branch)."""
  c = context()
  cp = c.capture_proxies
  if cp is not None and p is not None:
    q = cp.get(id(p))
    if q is not None:
      return q
  b = c.branch
  if b == 0 or p is None or not p.requires_grad or not USE_PROXIES[0] or b in c.no_proxy_branches:
    return p
  ent = c.proxies.get(id(p))
  if ent is None or ent[0] is not p:
    ent = (p, {})
    c.proxies[id(p)] = ent
  q = ent[1].get(b)
  if q is None or q.data_ptr() != p.data_ptr():
    q = p.detach().requires_grad_(True)
    ent[1][b] = q
  return q


def branch_leaf(p, index):
  """The autograd leaf branch `index` saw for parameter p (its alias, or p itself when the branch ran
  without aliases / never touched p)."""
  c = context()
  ent = c.proxies.get(id(p))
  if ent is None or ent[0] is not p or index in c.no_proxy_branches:
    return p
  return ent[1].get(index, p)


def branch_grads(p):
  """Gradients the side branches accumulated for parameter p (list, possibly empty)."""
  ent = context().proxies.get(id(p))
  if ent is None or ent[0] is not p:
    return []
  return [q.grad for q in ent[1].values() if q.grad is not None]


def fold_branch_grads(params):
  """p.grad += the gradients the side branches accumulated for p (and drop those): for callers that
  need ONE gradient per parameter before the optimiser -- e.g. a gradient all-reduce."""
  tgt, src = [], []
  for p in params:
    for g in branch_grads(p):
      if p.grad is None:
        p.grad = g.clone()
      else:
        tgt.append(p.grad)
        src.append(g)
  if tgt:
    torch._foreach_add_(tgt, src)
  clear_branch_grads()


def clear_branch_grads():
  for _, d in context().proxies.values():
    for q in d.values():
      q.grad = None


class branch(object):
  """Fork the enclosed forward onto a side stream / graph branch (see above).  Not re-entrant."""

  def __init__(self, index=1, proxies=True):
    assert index >= 1
    self.index = index
    self.proxies = proxies

  def __enter__(self):
    c = self.bctx = context()
    assert c.branch == 0, "branches do not nest"
    (c.no_proxy_branches.discard if self.proxies else c.no_proxy_branches.add)(self.index)
    dev = torch.cuda.current_device()
    key = (dev, self.index)
    self.main = torch.cuda.current_stream()
    st = c.streams.get(key)
    if st is None:
      # HIP multiplexes streams onto a few hardware queues: keep a side stream that really runs beside the
      # caller's and is not parked behind the process group's collectives (iic_amd.graph.pick_stream; a pair on
      # one queue would run the two views one after the other)
      from .graph import pick_stream
      st = c.streams[key] = pick_stream((self.main,), "side stream of ops.branch", collective_free=True)
    self.side = st
    st.wait_stream(self.main)                       # fork
    for _, d in c.proxies.values():                 # last step's branch gradients are consumed
      q = d.get(self.index)
      if q is not None:
        q.grad = None
    self.ctx = torch.cuda.stream(st)
    self.ctx.__enter__()
    c.branch = self.index
    c.branch_main = self.main
    return self

  def __exit__(self, *exc):
    c = self.bctx
    c.branch = 0
    c.branch_main = None
    self.ctx.__exit__(*exc)
    c.pending_join.append((self.main, self.side))   # joined later: the main view runs meanwhile
    if exc and exc[0] is not None:
      join()            # the forward raised: nobody downstream will join -- do not leave the fork pending
    return False


class on_branch(object):
  """Low-level: run the enclosed code as branch `index` on `stream` WITHOUT any fork / join
  synchronisation (iic_amd.graph.CapturedPairStep orders its per-view graphs itself)."""

  def __init__(self, index, stream):
    self.index, self.stream = index, stream

  def __enter__(self):
    c = self.bctx = context()
    assert c.branch == 0, "branches do not nest"
    # (this view sees the parameters through leaf aliases whatever an earlier auto_branch run left behind: with the
    #  index still marked alias-free, its gradients would be accumulated into .grad across the two streams)
    c.no_proxy_branches.discard(self.index)
    self.ctx = torch.cuda.stream(self.stream)
    self.ctx.__enter__()
    c.branch = self.index
    return self

  def __exit__(self, *exc):
    self.bctx.branch = 0
    self.ctx.__exit__(*exc)
    return False


# Automatic two-stream execution for UNCHANGED training scripts (IIC_AUTO_BRANCH=1; `python -m
# iic_amd.run` switches it on).  The reference's step calls net(all_imgs) and net(all_imgs_tf) one
# after the other (cluster_sobel.py:238-239, segmentation_twohead.py:300-306) and hands both
# results to the loss: the first training forward since the last join is put on the side stream,
# the second runs on the caller's stream meanwhile, and the loss (ours) joins.  No parameter
# aliases here -- autograd accumulates both views into p.grad, so any optimiser works.  Contract:
# the outputs of the first forward must not be consumed by anything but this library's losses
# before the join (true of every reference script); evaluation / no_grad forwards never branch.
# A forward of the pair that runs EAGERLY -- graph replay off, a warm-up occurrence, a shape that was not captured --
# stays on the caller's stream (BranchContext.solo_first); the two streams are for captured / replayed views, whose
# gradient hand-over is explicit (iic_amd/graphed.py).
AUTO_BRANCH = [os.environ.get("IIC_AUTO_BRANCH", "0") == "1"]
# forwards that hand back FEATURES (semisup heads: sup_head5.py:34-35, net6c_two_head.py:78-94,
# k-means feature extraction) are consumed by modules outside this library, which know nothing about
# the side stream: they never branch
_FEATURE_FLAGS = ("trunk_features", "penultimate_features", "kmeans_use_features")
# running-statistic updates postponed by branch forwards (ops.bn_finalize): flushed at every join; the
# optimiser and the losses join.  A caller that does neither would grow the list without bound and
# evaluate on stale running statistics -- past this many entries the next forward joins by itself.
_DEFERRED_LIMIT = 1024


class HeadPack(object):
  """What the sub-head outputs of ONE forward share: the reference hands the loss a python list of per-sub-head
  [bn, k] tensors (net5g.py:76-80) and calls IID_loss once per sub-head (cluster_sobel.py:241-253).  The list's
  tensors are tagged with their pack and index so that iic_amd.losses.IID_loss can evaluate all sub-head pairs of
  two packs in ONE set of launches at the first call and hand the other calls their share."""
  __slots__ = ("tensors", "cache", "__weakref__")

  def __init__(self, tensors):
    # weak references: a tensor -> pack -> tensor cycle would keep a step's autograd graph (and with it ~18 GB of
    # saved activations at the north-star batch) alive until the cyclic garbage collector happens to run
    self.tensors = [weakref.ref(t) for t in tensors]
    self.cache = {}

  def alive(self):
    ts = [r() for r in self.tensors]
    return ts if all(t is not None for t in ts) else None


def tag_pack(tensors):
  """Tag a list of per-sub-head output tensors (returns the list)."""
  if len(tensors) > 1 and all(torch.is_tensor(t) and t.dim() == 2 for t in tensors):
    pack = HeadPack(tensors)
    for i, t in enumerate(tensors):
      t._iic_pack = (pack, i)
  return tensors


# Graph replay of the training forwards / backwards for unchanged scripts (iic_amd/graphed.py);
# `python -m iic_amd.run` switches it on (IIC_GRAPH_FORWARD=0 keeps eager launches).
GRAPH_FORWARD = [os.environ.get("IIC_GRAPH_FORWARD", "0") == "1"]


def auto_branch(fwd):
  """Decorator for the architectures' forward()."""
  from . import pool        # (pool keys its buffers by current_branch(): it imports this module, not the reverse)

  def wrapped(self, x, *a, **k):
    c = context()
    if c.branch == 0 and (c.pending_join or c.deferred_running) and (
        not self.training or not torch.is_grad_enabled() or len(c.deferred_running) > _DEFERRED_LIMIT):
      join()      # evaluation must see up-to-date running statistics; bound the postponed list
    run = fwd
    will_branch = (AUTO_BRANCH[0] and self.training and torch.is_grad_enabled() and c.branch == 0
                   and not c.pending_join and not c.solo_first and torch.is_tensor(x) and x.is_cuda
                   and not any(k.get(f) for f in _FEATURE_FLAGS))
    pl = None
    if GRAPH_FORWARD[0]:
      from . import graphed
      if graphed.eligible(self, x, a, k):
        pl = graphed.plan(self, x, k, 1 if will_branch else c.branch)

        def run(self_, x_, *a_, **k_):      # captured-graph replay once this (shape, head, position) is warm
          return graphed.forward(fwd, self_, x_, a_, k_, pl)
    if will_branch:
      if pl is None or pl.mode == "eager":
        # eager launches stay on the caller's stream.  A planned position keeps its resource namespace (so that its
        # buffers exist before the capture) but sees the parameters themselves; the pair's second forward must not
        # fork in its place, and the running-statistic updates of both are applied at the join, in call order.
        c.solo_first = 1
        if pl is not None:
          c.no_proxy_branches.add(pl.res)
        try:
          return run(self, x, *a, **k)
        except BaseException:
          c.solo_first = 0              # the forward raised: there will be no second view to wait for
          raise
      # a replayed / captured view: side stream, the parameters themselves, gradients handed over by its autograd node
      with branch(proxies=False) as br:
        x.record_stream(br.side)         # allocated on the caller's stream, consumed on the side stream
        return run(self, x, *a, **k)
    if c.solo_first == 1 and self.training and torch.is_grad_enabled() and c.branch == 0:
      # the second view of a pair whose first view stayed on the caller's stream: its running-statistic updates are
      # postponed like the first view's (ops.bn_finalize) and the pair ends with it.  Both views ran on the caller's
      # stream, so nothing is left to wait for: the postponed updates are applied right here, in call order -- a
      # state_dict() / checkpoint taken after the step sees them whoever owns the loss and the optimiser
      try:
        return run(self, x, *a, **k)
      finally:
        join()
    if not torch.is_grad_enabled():
      mark = pool.POOL.mark()            # evaluation: nothing will release the activations later
      try:
        return fwd(self, x, *a, **k)
      finally:
        pool.POOL.sweep(mark)
    return run(self, x, *a, **k)
  wrapped.__name__ = getattr(fwd, "__name__", "forward")
  wrapped.__doc__ = fwd.__doc__
  wrapped.__wrapped__ = fwd          # inspect.signature() shows the architecture's own parameters
  return wrapped


def join():
  """Main stream waits for the side branches forked since the last join, then applies their
  postponed running-statistic updates (after the main view's own: sequential order)."""
  c = context()
  while c.pending_join:
    main, side = c.pending_join.pop()
    main.wait_stream(side)
  c.solo_first = 0
  flush_deferred_running()


BN_MOMENTUM = 0.1     # (ops.bn_finalize uses the same one for the updates it does not postpone)


def flush_deferred_running():
  """Apply the running-statistic updates the branch forwards postponed (one launch)."""
  deferred = context().deferred_running
  if not deferred:
    return
  items = list(deferred)
  del deferred[:]
  n = len(items)
  VP = ctypes.c_void_p * n
  IP = ctypes.c_int * n
  check(lib().iic_bn_running_update(
    n, VP(*[ptr(c) for c, _, _, _, _ in items]), VP(*[ptr(rm) for _, rm, _, _, _ in items]),
    VP(*[ptr(rv) for _, _, rv, _, _ in items]), VP(*[ptr(nb) for _, _, _, nb, _ in items]),
    IP(*[C for _, _, _, _, C in items]), BN_MOMENTUM, stream_ptr()), "iic_bn_running_update")


def branch_backward(fn):
  """Decorator for autograd Function.backward: run under the branch the forward recorded."""
  from .pool import PT_DTYPE

  def wrapped(ctx, *grads):
    if getattr(ctx, "_iic_ran", False):
      raise RuntimeError("iic_amd: backward through this graph a second time -- the saved activation "
                         "buffers went back to the pool after the first pass (retain_graph is not "
                         "supported on the HIP path)")
    ctx._iic_ran = True
    prev_dt = PT_DTYPE[0]
    PT_DTYPE[0] = getattr(ctx, "pt_dtype", prev_dt)     # (fp32_mode() forwards allocate fp32 in backward too)
    try:
      with context().as_branch(getattr(ctx, "branch", 0)):
        return fn(ctx, *grads)
    finally:
      PT_DTYPE[0] = prev_dt
  wrapped.__name__ = getattr(fn, "__name__", "backward")
  return staticmethod(wrapped)
