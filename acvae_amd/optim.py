"""The optimiser of ``TrainStep``: conf["optimizer"] / conf["optimizer_args"] of the reference
(``runners/pytorch_runner_vae.py:219-220``) resolved to one of the fused flat-buffer updates, and a
``torch.optim.Optimizer`` façade over it so that LR schedulers (torch's and the reference's ``utils/lr_scheduler``
classes) and the ``{"optimizer": optimizer.state_dict(), "lr_scheduler": scheduler.state_dict()}`` checkpoint work
against ``ts.optimizer`` unchanged.

Name and option resolution is host arithmetic and runs without a GPU.

Parameter groups (``TrainStep(param_groups=)``): ``resolve_groups`` turns torch's ``[{"params": ..., **overrides}]`` into full
group dicts and refuses what the fused update cannot vary per group, ``split_params`` is the common recipe (encoder at its
own learning rate, no weight decay on biases and normalisation scales), ``chunk_table`` cuts the flat buffer into the chunks
the grouped kernels walk."""
import inspect

import numpy as np
import torch

SUPPORTED = ("Adam", "AdamW", "SGD")
# hyperparameters of TrainStep's own keywords, by the optimiser they belong to
_KEYWORDS = {"Adam": ("lr", "betas", "eps", "weight_decay"), "AdamW": ("lr", "betas", "eps", "weight_decay"),
             "SGD": ("lr", "weight_decay")}
# what a param group may override; every other option of the torch class is structural (one value for the whole buffer)
PER_GROUP = {"Adam": ("lr", "betas", "eps", "weight_decay"), "AdamW": ("lr", "betas", "eps", "weight_decay"),
             "SGD": ("lr", "momentum", "weight_decay")}
MAX_GROUPS = 8                                  # ACVAE_OPT_MAX_GROUPS of include/acvae_hip.h
CHUNK_FIRST = 256                               # ACVAE_OPT_CHUNK_FIRST


def _dummy():
    return [torch.zeros(1, requires_grad=True)]


def check_group(name, group):
    """Options the fused update does not implement: ValueError naming the option."""
    for opt in ("maximize", "differentiable"):
        if group.get(opt):
            raise ValueError(f"{name}({opt}=True) is not supported by TrainStep's fused update")
    if name == "SGD" and group.get("nesterov") and (group.get("momentum", 0) == 0 or group.get("dampening", 0) != 0):
        raise ValueError("SGD(nesterov=True) requires momentum != 0 and dampening == 0")


def resolve(name, optimizer_args=None, **keywords):
    """-> the param-group hyperparameters of ``torch.optim.<name>`` (its ``defaults`` with the options applied).

    Defaults come from the torch class; ``keywords`` (TrainStep's ``lr=``, ``betas=``, ``eps=``, ``weight_decay=``; None
    = not given) override them and ``optimizer_args`` overrides both.  Raises ValueError for an unknown name, an option
    the class does not have, one the fused update does not implement, or a value torch itself refuses."""
    if name not in SUPPORTED:
        raise ValueError(f"optimizer {name!r} is not supported by TrainStep (supported: {', '.join(SUPPORTED)})")
    cls = getattr(torch.optim, name)
    known = cls(_dummy()).defaults
    opts = {}
    for k, v in keywords.items():
        if v is None:
            continue
        if k not in _KEYWORDS[name]:
            raise ValueError(f"{k}= is not an option of {name}")
        opts[k] = v
    args = dict(optimizer_args or {})
    for k in args:
        if k not in known:
            raise ValueError(f"{k!r} is not an option of torch.optim.{name}"
                             + (" (TrainStep's optimizer has exactly one param group)" if k == "params" else ""))
    opts.update(args)
    check_group(name, opts)
    group = dict(cls(_dummy(), **opts).defaults)       # torch validates the values (ranges, nesterov)
    if "betas" in group:
        group["betas"] = tuple(group["betas"])
    return group


def check_groups(name, groups):
    """What must hold across the groups on every step (schedulers and users write into the dicts): each group passes
    ``check_group``, the structural options agree, and SGD's momentum is zero in all groups or in none."""
    for i, g in enumerate(groups):
        try:
            check_group(name, g)
        except ValueError as e:
            raise ValueError(f"param group {i}: {e}") from None
        for k in structural_options(name):
            if k in g and k in groups[0] and g[k] != groups[0][k]:
                raise ValueError(f"param group {i}: {k}={g[k]!r} differs from group 0's {groups[0][k]!r}; {k} is one "
                                 "option for the whole flat buffer, not a per-group one")
    if name == "SGD" and len({float(g["momentum"]) != 0 for g in groups}) > 1:
        raise ValueError("SGD momentum is zero in some param groups and non-zero in others (the momentum buffer exists "
                         "for the whole flat buffer or not at all)")


_STRUCTURAL = {}


def structural_options(name):
    """The options of torch.optim.<name> that no group may override (amsgrad, nesterov, dampening, maximize, foreach, ...)."""
    if name not in _STRUCTURAL:
        _STRUCTURAL[name] = tuple(k for k in getattr(torch.optim, name)(_dummy()).defaults if k not in PER_GROUP[name])
    return _STRUCTURAL[name]


def resolve_groups(name, base, param_groups):
    """-> [{"params": [Parameter, ...], **hyperparameters}] for ``TrainStep(param_groups=)``: every group is ``base`` (what
    ``resolve`` returned) with the group's own overrides of ``PER_GROUP[name]``.  ValueError, naming the group and the key,
    for an empty list or more than ``MAX_GROUPS`` groups, a group without "params", a parameter listed twice, an unknown
    key, a structural option with another value than ``base``'s, a value torch's class refuses, and SGD momentum that is
    zero in some groups only.  Host arithmetic: nothing is built."""
    if isinstance(param_groups, dict) or not isinstance(param_groups, (list, tuple)):
        raise ValueError("param_groups must be a list of dicts {'params': ..., **overrides}")
    if not 1 <= len(param_groups) <= MAX_GROUPS:
        raise ValueError(f"param_groups must hold 1..{MAX_GROUPS} groups, not {len(param_groups)}")
    cls = getattr(torch.optim, name)
    accepted = set(inspect.signature(cls.__init__).parameters)
    seen, out = {}, []
    for i, g in enumerate(param_groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(f"param group {i}: not a dict with 'params'")
        ps = g["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for p in ps:
            if not isinstance(p, torch.nn.Parameter):
                raise ValueError(f"param group {i}: 'params' holds a {type(p).__name__}, not a Parameter")
            if id(p) in seen:
                raise ValueError(f"param group {i}: a parameter of shape {tuple(p.shape)} is already in group {seen[id(p)]}")
            seen[id(p)] = i
        full = dict(base)
        for k, v in g.items():
            if k == "params":
                continue
            if k not in base:
                raise ValueError(f"param group {i}: {k!r} is not an option of torch.optim.{name}")
            if k not in PER_GROUP[name]:
                if v != base[k]:
                    raise ValueError(f"param group {i}: {k}={v!r} differs from the optimizer's {base[k]!r}; only "
                                     f"{', '.join(PER_GROUP[name])} may vary per group")
                continue
            full[k] = tuple(v) if k == "betas" else v
        try:
            # torch validates the values (a default of the class that its constructor does not take is not passed)
            cls(_dummy(), **{k: v for k, v in full.items() if k in accepted})
        except (ValueError, TypeError) as e:
            raise ValueError(f"param group {i}: {e}") from None
        full["params"] = ps
        out.append(full)
    check_groups(name, out)
    return out


def check_coverage(groups, trainable, optional=()):
    """Every parameter of ``trainable`` (those the flat buffer updates) is in exactly one group; those of ``optional`` (the
    encoder's pooled head, which gets no gradient) may be left out.  ValueError otherwise."""
    listed = {id(p) for g in groups for p in g["params"]}
    free = {id(p) for p in optional}
    missing = [tuple(p.shape) for p in trainable if id(p) not in listed and id(p) not in free]
    if missing:
        raise ValueError(f"param_groups: {len(missing)} trainable parameter(s) are in no group (shapes {missing[:4]}"
                         f"{', ...' if len(missing) > 4 else ''})")


def split_params(model, encoder_lr=None, no_decay=True):
    """The common recipe as ``TrainStep(param_groups=)`` takes it: the encoder's parameters and the rest, each split into
    ``ndim >= 2`` (weights) and ``ndim <= 1`` (biases, normalisation scales and shifts).  The ``ndim <= 1`` groups get
    ``weight_decay=0.0`` (``no_decay``), the encoder groups ``lr=encoder_lr`` (None: the optimizer's).  Order: encoder
    weights, encoder rest, other weights, other rest; empty groups are dropped.  Frozen parameters are left out."""
    enc = {id(p) for p in model.encoder.parameters()}
    groups = []
    for in_enc in (True, False):
        for small in (False, True):
            ps = [p for p in model.parameters() if p.requires_grad and (id(p) in enc) == in_enc and (p.ndim <= 1) == small]
            if not ps:
                continue
            g = {"params": ps}
            if in_enc and encoder_lr is not None:
                g["lr"] = encoder_lr
            if small and no_decay:
                g["weight_decay"] = 0.0
            groups.append(g)
    return groups


def group_segments(sizes, group_of, skipped=(), first=()):
    """[(start, end, group, first)] in elements: the maximal runs of adjacent parameters that share a group, are not in
    ``skipped`` and agree on membership in ``first`` (indices into ``sizes``)."""
    skipped, first = set(skipped), set(first)
    segs, off = [], 0
    for i, (sz, g) in enumerate(zip(sizes, group_of)):
        if i not in skipped:
            f = i in first
            if segs and segs[-1][1] == off and segs[-1][2] == g and segs[-1][3] == f:
                segs[-1][1] = off + sz
            else:
                segs.append([off, off + sz, g, f])
        off += sz
    return [tuple(s) for s in segs]


def chunk_table(sizes, group_of, skipped, first, chunk):
    """-> int32 [n_chunks, 3], the table of acvae_grad_norm_groups / acvae_*_groups_step: rows (start / 4, length / 4,
    group | CHUNK_FIRST for a first SGD update), ascending, every segment of ``group_segments`` cut into chunks of at most
    ``chunk`` elements.  ``sizes``: the padded slice sizes in flat order; ``group_of``: each parameter's group; ``skipped`` /
    ``first``: indices of parameters without a gradient / whose SGD momentum buffer does not exist yet.  Refuses (ValueError)
    whatever the kernel would have to clamp or skip: a size that is no positive multiple of 4, a group outside
    0..MAX_GROUPS-1, a chunk size that is no positive multiple of 4, an index outside the list, a buffer of 2^33 elements
    or more.  Pure numpy."""
    sizes, group_of = [int(s) for s in sizes], [int(g) for g in group_of]
    if len(sizes) != len(group_of):
        raise ValueError(f"chunk_table: {len(sizes)} sizes, {len(group_of)} groups")
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk <= 0 or chunk % 4:
        raise ValueError(f"chunk_table: chunk must be a positive multiple of 4, not {chunk!r}")
    chunk = int(chunk)
    for i, (sz, g) in enumerate(zip(sizes, group_of)):
        if sz <= 0 or sz % 4:
            raise ValueError(f"chunk_table: size {sz} of parameter {i} is no positive multiple of 4")
        if not 0 <= g < MAX_GROUPS:
            raise ValueError(f"chunk_table: group {g} of parameter {i} is outside 0..{MAX_GROUPS - 1}")
    for what, idx in (("skipped", skipped), ("first", first)):
        for i in idx:
            if isinstance(i, bool) or int(i) != i or not 0 <= i < len(sizes):
                raise ValueError(f"chunk_table: {what} index {i!r} is outside the {len(sizes)} parameters")
    if sum(sizes) >= 1 << 33:
        raise ValueError("chunk_table: the buffer does not fit int32 float4 offsets")
    rows = []
    for a, b, g, f in group_segments(sizes, group_of, skipped, first):
        starts = np.arange(a, b, chunk, dtype=np.int64)
        lens = np.minimum(starts + chunk, b) - starts
        rows.append(np.stack([starts // 4, lens // 4, np.full_like(starts, g | (CHUNK_FIRST if f else 0))], axis=1))
    if not rows:
        return np.zeros((0, 3), dtype=np.int32)
    return np.ascontiguousarray(np.concatenate(rows).astype(np.int32))


class FlatOptimizer(torch.optim.Optimizer):
    """``torch.optim.Optimizer`` over ``model.parameters()`` (one param group, as the reference builds it) whose update
    is TrainStep's fused pass over the flat buffer.  ``step()`` is called by ``TrainStep.step`` through the instance
    attribute, so LR schedulers see it as they see a torch optimiser's step; called on its own it raises (the update
    needs the gradients and the device-side norm of the step that TrainStep is running).  The hyperparameters are read
    from ``param_groups[0]`` on every step: schedulers may change ``lr`` and ``momentum`` / ``betas``.
    ``state_dict()`` / ``load_state_dict()`` use the layout of ``torch.optim.<name>``.

    With ``TrainStep(param_groups=)`` ``params`` is the list of group dicts ``resolve_groups`` made: ``param_groups`` then
    holds those G groups, every one of them read on every step, and schedulers that take one value per group
    (``LambdaLR`` with a list of functions, ``OneCycleLR`` with a list of ``max_lr``) drive them.  Groups cannot be added
    after construction."""

    def __init__(self, owner, params, name, group):
        self._owner, self.name = owner, name
        self._built = False
        super().__init__(list(params), group)
        self._built = True

    def add_param_group(self, param_group):
        if self._built:
            raise ValueError("TrainStep's optimizer has exactly one param group (over model.parameters()) unless "
                             "TrainStep(param_groups=) names them; none can be added after construction")
        super().add_param_group(param_group)

    def step(self, closure=None):
        if closure is not None:
            raise ValueError("TrainStep's optimizer takes no closure")
        self._owner._apply_update()

    def state_dict(self):
        return self._owner.optimizer_state_dict()

    def load_state_dict(self, state_dict):
        self._owner.load_optimizer_state_dict(state_dict)
