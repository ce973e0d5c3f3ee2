"""Optimizer `bert_adam` (expt/nytimes/9_transformer_objects/config.yaml:126-149) as one
multi-tensor HIP kernel over flat fp32 buffers.  Update rule restated from
pytorch_pretrained_bert.BertAdam (third-party, absent here; parity unpinned):
per-tensor gradient-norm clipping, no bias correction, decoupled-style weight decay added
to the update, `warmup_linear` schedule evaluated at the step count BEFORE the increment."""
import ctypes
import math
import re
import warnings

import torch

from .. import hip
from .. import runtime as rt


def warmup_linear(progress, warmup):
    """pytorch_pretrained_bert WarmupLinearSchedule.get_lr_"""
    if progress < warmup:
        return progress / warmup
    return max((progress - 1.0) / (warmup - 1.0), 0.0)


# what a parameter group may override, in the order of a row of tell_bertadam_step_groups' table (include/tell_hip.h)
GROUP_KEYS = ('lr', 'warmup', 't_total', 'b1', 'b2', 'e', 'weight_decay', 'max_grad_norm')
MAX_GROUPS = 16


def resolve_parameter_groups(names, defaults, parameter_groups):
    """AllenNLP's `parameter_groups` ([[regex, ...], {overrides}] per group) over the tensor names of a FlatParams.
    A tensor belongs to the FIRST listed group of which any regex matches its name (re.search); one that no regex matches
    belongs to the default group, which carries `defaults` (the constructor's own eight values).  A group inherits what
    it does not override; listed groups that end up empty are dropped; groups whose eight values are equal are merged.
    -> (groups, tensor_group): groups a list of dicts (GROUP_KEYS + 'names'), listed ones first in their order, the
    default group last; tensor_group[i] the index into it of names[i]."""
    listed = []
    for gi, entry in enumerate(parameter_groups or []):
        try:
            regexes, overrides = entry
            regexes, overrides = list(regexes), dict(overrides)
        except (TypeError, ValueError):
            raise ValueError('bert_adam: parameter_groups[%d] must be [[regex, ...], {overrides}], got %r' % (gi, entry))
        values = dict(defaults)
        for key, value in overrides.items():
            where = 'bert_adam: parameter_groups[%d], key %r: ' % (gi, key)
            if key == 'schedule':
                if value != 'warmup_linear':
                    raise ValueError(where + "only 'warmup_linear' is implemented, got %r" % (value,))
                continue
            if key not in GROUP_KEYS:
                raise ValueError(where + 'not a key a group can override (%s)' % ', '.join(GROUP_KEYS))
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
                raise ValueError(where + 'must be a finite number, got %r' % (value,))
            if key == 'e' and not ctypes.c_float(value).value > 0:
                raise ValueError(where + 'must be positive as an fp32 number, got %r' % (value,))
            if key in ('b1', 'b2') and not 0.0 <= value <= 1.0:
                raise ValueError(where + 'must be in [0, 1], got %r' % (value,))
            values[key] = value
        listed.append((regexes, values))
    used = {rx: False for regexes, _ in listed for rx in regexes}
    members = [[] for _ in listed] + [[]]
    for name in names:
        home = len(listed)
        for gi, (regexes, _) in enumerate(listed):
            hit = [rx for rx in regexes if re.search(rx, name)]
            for rx in hit:
                used[rx] = True
            if hit and home == len(listed):
                home = gi
        members[home].append(name)
    for rx, hit in used.items():
        if not hit:
            warnings.warn('bert_adam: the parameter_groups regex %r matches no trainable tensor' % (rx,))
    groups, index, group_of = [], {}, {}
    for (_, values), mine in zip(listed + [(None, dict(defaults))], members):
        if not mine:
            continue
        key = tuple(float(values[k]) for k in GROUP_KEYS)
        if key not in index:
            index[key] = len(groups)
            groups.append(dict(values, names=[]))
        for name in mine:
            group_of[name] = index[key]
    if len(groups) > MAX_GROUPS:
        raise ValueError('bert_adam: parameter_groups resolve to %d distinct groups, the step kernel takes %d' %
                         (len(groups), MAX_GROUPS))
    for name in names:          # (a merged group keeps its tensors in the order of `names`)
        groups[group_of[name]]['names'].append(name)
    return groups or [dict(defaults, names=[])], [group_of[name] for name in names]


class FlatParams:
    """Trainable parameters re-homed into one flat fp32 buffer (+ matching grad / m / v
    buffers).  Every tensor starts on a CHUNK boundary so a chunk belongs to one tensor
    (per-tensor norms without atomics); `p.data` and `p.grad` become views."""

    def __init__(self, named_params, device):
        chunk = hip.lib().tell_opt_chunk()
        self.names, self.params, offs = [], [], []
        total = 0
        seen = set()
        for name, p in named_params:
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            self.names.append(name)
            self.params.append(p)
            offs.append(total)
            total += (p.numel() + chunk - 1) // chunk * chunk
        self.total, self.chunk, self.offsets = total, chunk, offs
        self.n_chunks = total // chunk
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.m = torch.zeros(total, dtype=torch.float32, device=device)
        self.v = torch.zeros(total, dtype=torch.float32, device=device)
        chunk_tensor = torch.empty(self.n_chunks, dtype=torch.int32)
        begins = []
        for i, (p, o) in enumerate(zip(self.params, offs)):
            n = p.numel()
            self.flat[o:o + n].copy_(p.data.reshape(-1).to(device=device, dtype=torch.float32))
            p.data = self.flat[o:o + n].view(p.shape)
            g = self.grad[o:o + n].view(p.shape)
            p.grad = g
            p._tell_grad = g
            c0, c1 = o // chunk, (o + (n + chunk - 1) // chunk * chunk) // chunk
            chunk_tensor[c0:c1] = i
            begins.append(c0)
        begins.append(self.n_chunks)
        self.chunk_tensor = chunk_tensor.to(device)
        self.chunk_begin = torch.tensor(begins, dtype=torch.int64, device=device)
        # bf16 working copy of every parameter, rewritten by the optimizer kernel itself (ops.weight reads it)
        self.shadow = None
        if torch.device(device).type == 'cuda':
            self.shadow = torch.empty(total, dtype=torch.bfloat16, device=device)
            for p, o in zip(self.params, offs):
                p._tell_shadow = self.shadow[o:o + p.numel()].view(p.shape)
            self.refresh_shadow()
        # tensors whose gradient the optimizer's zeroing leaves alone (their single dense producer stores over it:
        # ops.py 'Gradient stores'); all zero until the trainer has observed a step (set_grad_store)
        self.keep_grad = torch.zeros(max(len(self.params), 1), dtype=torch.int32, device=device)
        self.stored_numel = 0
        # True while the buffer holds gradients of defer_update passes that no update has consumed (trainer.py
        # _grad_store_begin: the pass that ends the accumulation must add to them, not store over part of them)
        self.accum_pending = False
        self.partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float32, device=device)
        self.norms = torch.zeros(len(self.params), dtype=torch.float32, device=device)
        # exponential moving average of the masters and the device scalar 1 - d_t of the current step: allocated by
        # enable_ema (BertAdam(ema_decay=...)), absent otherwise
        self.ema = self.ema_omd = None
        # device int32[n_tensors], the parameter group of every tensor: only with more than one group (set_tensor_group)
        self.tensor_group = None
        rt.bump_weights_epoch()

    def set_tensor_group(self, tensor_group):
        assert len(tensor_group) == len(self.params)
        self.tensor_group = torch.tensor(list(tensor_group), dtype=torch.int32).to(self.flat.device)

    def enable_ema(self):
        if self.ema is None:
            self.ema = self.flat.clone()
            self.ema_omd = torch.zeros(1, dtype=torch.float32, device=self.flat.device)

    def refresh_shadow(self):
        """Re-derive the bf16 working copy from the fp32 masters (after anything but the optimizer kernel wrote the
        flat buffer: construction, the initial DP broadcast, a checkpoint load into `flat`)."""
        if self.shadow is not None:
            hip.call('tell_cast', self.flat, hip.F32, self.shadow, hip.BF16, self.total)
            for p in self.params:
                p._tell_shadow_version = p._version

    def zero_grad(self):
        hip.call('tell_fill_f32', self.grad, self.total, 0.0)
        self.accum_pending = False

    def set_grad_store(self, seen):
        """seen: ops.grad_store_observe(False) of one whole backward pass - {id(p): (p, [(r0, r1) | None, ...])}, a None
        entry being an accumulating writer.  A parameter whose gradient rows were written exactly once each, by dense
        products only, is marked `_tell_grad_store` (and kept out of the optimizer's zeroing).  -> elements marked."""
        flags = []
        for p in self.params:
            e = seen.get(id(p))
            ok = e is not None and e[0] is p and len(e[1]) > 0 and all(w is not None for w in e[1])
            if ok:
                pos = 0
                for r0, r1 in sorted(e[1]):
                    ok = ok and r0 == pos
                    pos = r1
                ok = ok and pos == p.shape[0]
            p._tell_grad_store = bool(ok)
            flags.append(int(ok))
        # the (g, v) pair of a GehringLinear is written by ONE launch with ONE store bit (ops._wn_backward): mark jointly
        index = {n: i for i, n in enumerate(self.names)}
        for n, ia in index.items():
            if n.endswith('.weight_g') and n[:-1] + 'v' in index:
                ib = index[n[:-1] + 'v']
                if flags[ia] != flags[ib]:
                    flags[ia] = flags[ib] = 0
                    self.params[ia]._tell_grad_store = self.params[ib]._tell_grad_store = False
        if flags:
            self.keep_grad.copy_(torch.tensor(flags, dtype=torch.int32))
        self.stored_numel = sum(p.numel() for p, f in zip(self.params, flags) if f)
        return self.stored_numel

    def numel(self):
        return sum(p.numel() for p in self.params)


class BertAdam:
    def __init__(self, flat, lr=1e-4, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999,
                 e=1e-6, weight_decay=0.01, max_grad_norm=1.0, parameter_groups=None, ema_decay=None, ema_warmup=10.0):
        """parameter_groups: AllenNLP's [[regex, ...], {overrides}] list over flat.names (resolve_parameter_groups); with
        more than one distinct group the step is tell_bertadam_step_groups - still one update launch, the hyperparameters
        looked up per chunk - and with one it is the launch it always was.
        ema_decay (None: off): keep an exponential moving average of the fp32 masters in flat.ema, updated by the step
        kernel itself with the decay d_t = min(ema_decay, (1 + n) / (ema_warmup + n)) after n applied updates
        (ema_warmup <= 0: always ema_decay); csrc/optim.hip, DESIGN.md section 31."""
        assert schedule == 'warmup_linear'
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or \
                    not (math.isfinite(ema_decay) and 0.0 <= ema_decay < 1.0):
                raise ValueError('bert_adam: ema_decay must be a number in [0, 1) or None, got %r' % (ema_decay,))
            if isinstance(ema_warmup, bool) or not isinstance(ema_warmup, (int, float)) or \
                    not (math.isfinite(ema_warmup) and ema_warmup >= 0.0):
                raise ValueError('bert_adam: ema_warmup must be a finite number >= 0, got %r' % (ema_warmup,))
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        # True while Trainer.ema_weights() has exchanged the masters with the average: no update may run then
        self.ema_swapped = False
        self._warned = set()
        self.flat = flat
        self.lr, self.warmup, self.t_total = lr, warmup, t_total
        self.b1, self.b2, self.e, self.weight_decay, self.max_grad_norm = b1, b2, e, weight_decay, max_grad_norm
        self.step_count = 0         # optimisation steps ISSUED by the host (incl. steps the device skipped)
        dev = flat.flat.device
        defaults = dict(zip(GROUP_KEYS, (lr, warmup, t_total, b1, b2, e, weight_decay, max_grad_norm)))
        self.groups, tensor_group = resolve_parameter_groups(flat.names, defaults, parameter_groups)
        self._group_of = dict(zip(flat.names, tensor_group))
        self.group_hp = None
        if len(self.groups) > 1:        # the table of tell_bertadam_step_groups, a host array that it takes by value
            flat.set_tensor_group(tensor_group)
            self.group_hp = (ctypes.c_float * (len(GROUP_KEYS) * len(self.groups)))(
                *[float(g[k]) for g in self.groups for k in GROUP_KEYS])
        self.lr_dev = torch.zeros(len(self.groups), dtype=torch.float32, device=dev)     # one per group
        # updates APPLIED: advanced by the update kernel itself, only when the step is not skipped for a non-finite
        # loss / gradient; the learning rate of a step is computed from it on the device (csrc/optim.hip)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.parameter_groups = parameter_groups
        if ema_decay is not None:
            flat.enable_ema()

    def reset_ema(self):
        """The average restarts from the current masters (after anything but the step kernel wrote them: the initial
        data-parallel broadcast, a checkpoint without an average)."""
        if self.ema_decay is None:
            raise ValueError('bert_adam: reset_ema() needs ema_decay (got ema_decay=None)')
        self.flat.ema.copy_(self.flat.flat)

    def _warn_once(self, text):
        if text not in self._warned:
            self._warned.add(text)
            warnings.warn(text)

    def applied_steps(self):
        """Updates applied so far = issued steps minus the skipped ones (one host sync)."""
        return int(self.step_dev.item())

    def group_of(self, name):
        """index into self.groups of the tensor called `name` (one of flat.names)"""
        return self._group_of[name]

    def current_lr(self, step=None, group=None):
        """Learning rate of the step that follows `step` applied updates (default: the host's count of issued steps;
        pass applied_steps() for what the device will actually use after skipped batches).  group: an index into
        self.groups, or a regex - the group of the tensors whose names it matches; needed once there are several groups."""
        step = self.step_count if step is None else step
        if group is None:
            if len(self.groups) > 1:
                raise ValueError('bert_adam: there are %d parameter groups - current_lr() needs group=, a group index or '
                                 'a regex over the tensor names' % len(self.groups))
            group = 0
        if isinstance(group, str):
            hits = sorted({g for name, g in self._group_of.items() if re.search(group, name)})
            if len(hits) != 1:
                raise ValueError('bert_adam: the regex %r matches tensors of %d groups (%s), not of one' %
                                 (group, len(hits), hits))
            group = hits[0]
        g = self.groups[group]
        lr, warmup, t_total = g['lr'], g['warmup'], g['t_total']
        if t_total != -1:
            return lr * warmup_linear(step / t_total, warmup)
        return lr

    def step(self, grad_scale=1.0, zero_grad=False, skip=None, grad_wire=None):
        """zero_grad: also clear the gradient buffer (fused into the update pass).  skip: device int32[2] flag -
        a non-zero skip[0] (non-finite loss / gradient) turns the step into gradient zeroing only."""
        self.prepare()
        self.launch(grad_scale, zero_grad, skip, grad_wire)
        self.advance()

    # the three parts of step(), separable so that the kernel launches can live in a captured graph
    def prepare(self):
        """Host part before the kernels: nothing any more - the schedule lives on the device (step_dev)."""

    def launch(self, grad_scale=1.0, zero_grad=False, skip=None, grad_wire=None):
        """grad_wire: optional bf16 copy of the whole flat gradient (the data-parallel exchange's wire buffer after the
        all-reduce): the kernels read it in place of flat.grad - no pass that widens it back first."""
        f = self.flat
        if self.ema_swapped:
            raise RuntimeError('bert_adam: no optimizer step inside Trainer.ema_weights() - the masters sit in the '
                               'EMA buffer')
        from .. import ops
        keep = f.keep_grad if (zero_grad and ops.grad_store_on()) else None
        if zero_grad:
            f.accum_pending = False
        if len(self.groups) > 1:
            ema = self.ema_decay is not None
            hip.call('tell_bertadam_step_groups', f.flat, f.grad, f.m, f.v, f.chunk_tensor, f.chunk_begin, f.n_chunks,
                     len(f.params), f.partial, f.norms, self.lr_dev, f.tensor_group, self.group_hp, len(self.groups),
                     float(grad_scale), f.shadow, int(zero_grad), skip, grad_wire, self.step_dev, keep,
                     f.ema if ema else None, f.ema_omd if ema else None, float(self.ema_decay) if ema else 0.0,
                     float(self.ema_warmup) if ema else 0.0)
            return
        g = self.groups[0]          # (the constructor's own values, unless one overriding group holds every tensor)
        args = (f.flat, f.grad, f.m, f.v, f.chunk_tensor, f.chunk_begin, f.n_chunks,
                len(f.params), f.partial, f.norms, self.lr_dev, g['b1'], g['b2'], g['e'], g['weight_decay'],
                g['max_grad_norm'], float(grad_scale), f.shadow, int(zero_grad), skip, grad_wire,
                self.step_dev, float(g['lr']), float(g['warmup']), float(g['t_total']), keep)
        if self.ema_decay is None:
            hip.call('tell_bertadam_step2', *args)
        else:
            hip.call('tell_bertadam_step_ema', *args, f.ema, f.ema_omd, float(self.ema_decay), float(self.ema_warmup))

    def advance(self):
        """Host part after the kernels.  The host cannot see a device-side skip without a synchronisation, so it bumps
        the weights epoch regardless: after a skipped step that costs one needless rebuild of the cached working
        weights in the eager schedule (the step graph rebuilds them inside the graph anyway) - never a stale one."""
        self.step_count += 1
        rt.bump_weights_epoch()

    def state_dict(self):
        sd = {'step': self.applied_steps(), 'm': self.flat.m, 'v': self.flat.v}
        if self.ema_decay is not None:
            sd['ema'] = self.flat.ema
        return sd

    def load_state_dict(self, sd):
        """The weights themselves travel with the model's state dict - load that first: a state without 'ema' restarts
        the average from the masters as they are now."""
        self.step_count = sd['step']
        self.step_dev.fill_(int(sd['step']))
        self.flat.m.copy_(sd['m'])
        self.flat.v.copy_(sd['v'])
        if self.ema_decay is not None:
            if 'ema' in sd:
                self.flat.ema.copy_(sd['ema'])
            else:
                self._warn_once("bert_adam: the loaded state has no 'ema' - the average restarts from the loaded weights")
                self.reset_ema()
        elif 'ema' in sd:
            self._warn_once("bert_adam: the loaded state has an 'ema' but ema_decay is None - ignored")


def apply_no_grad(model, patterns):
    """trainer `no_grad` regex list (config.yaml:150-152)."""
    for name, p in model.named_parameters():
        if any(re.search(rx, name) for rx in patterns):
            p.requires_grad_(False)
