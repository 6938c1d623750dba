"""Invalidation of the packed device copies of weights (bf16 GEMM operands, fused adaLN matrices, decoder fragments).

A class that keeps device copies of weights derives from `PackedWeights` (listed in front of nn.Module) and implements `_pack`.
The mixin stamps every pack with the global weights EPOCH; anything that changes parameters bumps the epoch: `load_state_dict`
anywhere in a tree that holds a cache (post-hooks, which also fire when a strict load raises), `Module._apply` (.to / .cuda), and
the in-place writers of this package (`parallel.broadcast_flat`, `synth.fill_module_random_`, `checkpoint.load_checkpoint`).
Callers that write parameters in place themselves call `ln3diff_amd.invalidate_weight_caches()`.  So do callers that REPLACE a submodule
of a holder after its first forward (`dit.blocks[3] = other`): the load hooks sit on the submodules that existed when the cache was stamped
(`watch_tree`), the new module has none, and assigning it is no parameter write - the holder keeps serving the old child's packed copies,
and a state dict loaded into the new child later goes unseen, until the epoch moves.

What a holder hands to its caller to pass back in (DiT `prepare_context` / `prepare_timesteps`) carries the epoch of the weights it was made
from; forward refuses it under any other epoch.  The epoch is global: a load into an unrelated module invalidates too - the conservative
rule, the same for the packed copies.
"""
import torch

EPOCH = [0]


def bump(*_a, **_k):
    EPOCH[0] += 1


def stamp(cache, owner=None):
    """Mark a freshly built cache with the current epoch.  `owner` (the module the cache belongs to) gets the load hook on EVERY
    submodule it has by now, so that a state dict loaded straight into a child (`dit.blocks[3].load_state_dict(...)`) also drops
    the parent's packed copies - the hook registered in the holder's __init__ only sees loads that go through the holder."""
    cache['epoch'] = EPOCH[0]
    if owner is not None:
        watch_tree(owner)
    return cache


def fresh(cache, device=None):
    return cache is not None and cache.get('epoch') == EPOCH[0] and (device is None or cache.get('device') == device)


def watch_tree(module):
    """Load hook on every submodule `module` has NOW; one that replaces a child later is not covered (module docstring)."""
    for sub in module.modules():
        if not sub.__dict__.get('_ln3d_watched', False):
            sub.register_load_state_dict_post_hook(bump)
            sub.__dict__['_ln3d_watched'] = True
    return module


def watch(module):
    """Load hook on `module` alone (PackedWeights.__init__: before the holder has children): weights loaded into it, or into a parent,
    drop every cache - also when it has never packed."""
    if not module.__dict__.get('_ln3d_watched', False):
        module.register_load_state_dict_post_hook(bump)
        module.__dict__['_ln3d_watched'] = True
    return module


def _norm(dev):
    """One name per device: a bare 'cuda' is the current device.  torch.cuda is touched for that form only."""
    if not isinstance(dev, torch.device):
        dev = torch.device(dev)
    if dev.index is None and dev.type == 'cuda':
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


class PackedWeights:
    """Mixin, listed in front of nn.Module, of every class that keeps device copies of its weights.  The holder implements
    `_pack(self, P, dev)`: fill the dict P with the copies for `dev` and, at its end, build the scratch that goes with them (Workspace,
    ConvStack).  Everything else is here and nowhere else: a pack is fresh while the epoch and the device it was built under hold
    (P['epoch'], taken after the build, and P['device']); a rebuild puts the load hook on every submodule there is by then; .to() /
    .cuda() / .float() bump the epoch; a state dict loaded into a holder that never packed bumps it too."""
    _packed = None

    def __init__(self, *a, **k):            # reached through the holder's super().__init__()
        super().__init__(*a, **k)
        watch(self)

    def _apply(self, fn, *a, **k):
        bump()
        return super()._apply(fn, *a, **k)

    def _ensure_packed(self, dev):
        """the pack for `dev`, rebuilt if the weights or the device changed since it was made"""
        if not fresh(self._packed, dev):            # per forward: one lookup, two compares (a bare 'cuda' also pays _norm, every time)
            dev = _norm(dev)
            if not fresh(self._packed, dev):
                P = {'device': dev}
                self._pack(P, dev)
                self._packed = stamp(P, self)
        return self._packed

    def _side_pack(self, name, dev, build):
        """A small pack of its own next to the main one, made on first use (operands of a seam that most callers never run):
        {'device', 'epoch', **build(dev)}, under the same freshness rule."""
        dev = _norm(dev)
        side = self.__dict__.setdefault('_side_packs', {})
        if not fresh(side.get(name), dev):
            side[name] = stamp({'device': dev, **build(dev)}, self)
        return side[name]
