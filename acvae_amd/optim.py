"""The optimiser of ``TrainStep``: conf["optimizer"] / conf["optimizer_args"] of the reference
(``runners/pytorch_runner_vae.py:219-220``) resolved to one of the fused flat-buffer updates, and a
``torch.optim.Optimizer`` façade over it so that LR schedulers (torch's and the reference's ``utils/lr_scheduler``
classes) and the ``{"optimizer": optimizer.state_dict(), "lr_scheduler": scheduler.state_dict()}`` checkpoint work
against ``ts.optimizer`` unchanged.

Name and option resolution is host arithmetic and runs without a GPU."""
import torch

SUPPORTED = ("Adam", "AdamW", "SGD")
# hyperparameters of TrainStep's own keywords, by the optimiser they belong to
_KEYWORDS = {"Adam": ("lr", "betas", "eps", "weight_decay"), "AdamW": ("lr", "betas", "eps", "weight_decay"),
             "SGD": ("lr", "weight_decay")}


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


class FlatOptimizer(torch.optim.Optimizer):
    """``torch.optim.Optimizer`` over ``model.parameters()`` (one param group, as the reference builds it) whose update
    is TrainStep's fused pass over the flat buffer.  ``step()`` is called by ``TrainStep.step`` through the instance
    attribute, so LR schedulers see it as they see a torch optimiser's step; called on its own it raises (the update
    needs the gradients and the device-side norm of the step that TrainStep is running).  The hyperparameters are read
    from ``param_groups[0]`` on every step: schedulers may change ``lr`` and ``momentum`` / ``betas``.
    ``state_dict()`` / ``load_state_dict()`` use the layout of ``torch.optim.<name>``."""

    def __init__(self, owner, params, name, group):
        self._owner, self.name = owner, name
        super().__init__(list(params), group)

    def add_param_group(self, param_group):
        if getattr(self, "param_groups", None):
            raise ValueError("TrainStep's optimizer has exactly one param group (over model.parameters())")
        super().add_param_group(param_group)

    def step(self, closure=None):
        if closure is not None:
            raise ValueError("TrainStep's optimizer takes no closure")
        self._owner._apply_update()

    def state_dict(self):
        return self._owner.optimizer_state_dict()

    def load_state_dict(self, state_dict):
        self._owner.load_optimizer_state_dict(state_dict)
