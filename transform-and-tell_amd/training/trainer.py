"""The optimisation step of tell/training/callback_apex_trainer.py:208-247 on the MI355X path,
data-parallel over one process per GPU (new functionality - the reference never runs
multi-process).

  zero_grad -> forward (model(**batch)) -> backward -> [RCCL all-reduce of the flat fp32
  gradient buffer over xGMI] -> BertAdam.

bf16 compute with fp32 master weights replaces apex amp O2 (no loss scaling needed).
DP equivalence with a single-GPU run on the concatenated batch: every rank's loss is
re-weighted by n_local*world/n_global (token counts all-reduced on the device) before
backward, then gradients are averaged.  Ranks that see no target of a tail cluster still
contribute zeros: the flat buffer is always reduced as a whole."""
import contextlib
import os

import torch

from .. import hip, ops, streams
from .. import runtime as rt
from ..common.registrable import Registrable
from . import dp
from .optimizers import BertAdam, FlatParams, apply_no_grad


class TrainerBase(Registrable):
    pass


class Trainer:
    def __init__(self, model, optimizer_cfg=None, no_grad=(r'^resnet', r'^roberta'), device='cuda',
                 nan_check=False, bucket_mb=256, async_update=None, allreduce_dtype=None, data_parallel=None,
                 capture_after=None, shape_buckets=(128, 16)):
        """nan_check=True: the reference's host-synchronous NaN test (returns None for a skipped batch, no step graph);
        the default skips non-finite steps on the device instead (self.skip, skipped_steps()).

        capture_after: sightings of a batch shape before its step / encoder graphs are captured (default
        graphs.CAPTURE_AFTER = 2; fixed-shape runs pass 1).  shape_buckets = (article, caption): when graphs are in
        use, article ids are right-padded (pad id) to a multiple of `article` tokens and captions to a multiple of
        `caption`, faces to 4 and objects to 64 NaN rows - a handful of shapes instead of one per batch.  Padding is
        invisible to the loss: padded keys are masked in every attention, padded targets are ignore_index, the
        DynamicConv is causal.  None: leave batches as the iterator made them."""
        import torch.distributed as dist
        # data_parallel=False: a single-process trainer even though a process group exists (equivalence tests)
        self.dist = dist if (dist.is_available() and dist.is_initialized() and data_parallel is not False) else None
        self.world = self.dist.get_world_size() if self.dist else 1
        # TELL_DP_SELFTEST=1: run every collective of the data-parallel path even in a 1-rank group (single-GPU check
        # of the RCCL calls, the streams they are issued on and their ordering)
        self.dp = self.world > 1 or (self.dist is not None and os.environ.get('TELL_DP_SELFTEST') == '1')
        self.rank = self.dist.get_rank() if self.dist else 0
        self.model = model.to(device)
        apply_no_grad(model, no_grad)
        if hasattr(model, 'reset_graphs'):           # requires_grad flags decide where the working weight copies live
            model.reset_graphs()
        self.flat = FlatParams(model.named_parameters(), device)
        cfg = dict(lr=1e-4, warmup=0.05, t_total=437600, schedule='warmup_linear', b1=0.9, b2=0.98, e=1e-6,
                   weight_decay=1e-5, max_grad_norm=0.1)                 # config.yaml:126-136
        cfg.update(optimizer_cfg or {})
        cfg.pop('type', None)
        self.optimizer = BertAdam(self.flat, **cfg)
        self.nan_check = nan_check
        self.bucket_elems = bucket_mb * (1 << 20) // 4
        self.batch_num_total = 0
        # gradients travel in bf16 when the model computes in bf16 (dp.all_reduce_flat_bf16), in fp32 in parity mode
        if allreduce_dtype is None:
            allreduce_dtype = torch.bfloat16 if (rt.compute_dtype() == torch.bfloat16 and
                                                 torch.device(device).type == 'cuda' and
                                                 os.environ.get('TELL_ALLREDUCE_FP32') != '1') else torch.float32
        self.allreduce_dtype, self._wire = allreduce_dtype, None
        if self.dp and self.world > 1:
            # RCCL's channel kernels will hold compute units while the next batch's encoders run: the 256x256 GEMMs
            # (csrc/gemm_q4.hip, one workgroup per CU) then take their tiles from per-XCD counters, so that a workgroup
            # whose CU is taken gets fewer tiles instead of finishing a static share late.  MEASURED on one GPU with N
            # CUs held by idle workgroups (bench.py --cu-hog N, profiles/r04_cu_hog.txt): configs[2] 1565 -> 1423 samples/s
            # with static tile lists for N = 8 / 16 / 32, -> 1498-1514 with the counters (1570 with no CU held).
            if 'TELL_Q4_DYNAMIC' not in os.environ:           # (an explicit choice at load time stands)
                hip.set_option('q4_dynamic', 1)
        # The step's long bandwidth-bound launches (BertAdam and its norm pass, the layer mix, the multi weight-norm
        # launches) fill all 256 CUs while they run, and the next batch's RoBERTa GEMMs - one workgroup per CU - cannot
        # start a tile meanwhile.  On the GPU the trainer issues them in the narrow form on at most 128 CUs (csrc/common.h,
        # same results bit for bit) and lets the GEMMs claim their tiles from the per-XCD counters,
        # so that they take whatever CUs are free.  MEASURED (bench.py, profiles/narrow_bw_bench.txt): 20.23 -> 19.62 ms per
        # step.  Scoped to the train_one_batch calls that get a next_batch (launches recorded into the step / encoder
        # graphs keep the choice they were captured with); an explicit TELL_BW_WGS / TELL_Q4_DYNAMIC at load time stands.
        self._lib_options = {}
        if torch.device(device).type == 'cuda':
            for key, value in (('bw_wgs', 128), ('q4_dynamic', 1)):
                if 'TELL_' + key.upper() not in os.environ:
                    self._lib_options[key] = value
        if self.dp:
            # every rank draws its own dropout masks: the counter-hash seed is process-global with the same default on
            # all ranks; the rank is mixed in where the seed is READ (runtime.seed), not written into the global seed
            rt.set_rank(self.rank)
        if self.dp:                           # identical initial weights on every rank
            self.dist.broadcast(self.flat.flat, src=0)
            self.flat.refresh_shadow()
            rt.bump_weights_epoch()
        # the optimizer was built before that broadcast: an average taken then would differ between ranks.  From here on
        # every rank computes the same average from the same reduced gradients - no communication
        if self.optimizer.ema_decay is not None:
            self.optimizer.reset_ema()
        # TELL_ASYNC_UPDATE=1: gradient all-reduce + BertAdam + gradient zeroing run on their own stream and the model
        # waits for it right before its first trainable weight (rt.wait_weight_update).  Off by default: with the
        # encoders of the next batch already running on their two streams, a fourth / fifth stream of ours costs more
        # in hardware-queue sharing than the overlap returns (streams.py: 1149 vs 1134 vs 1061 samples/s for
        # 3 / 4 / 5 streams)
        if async_update is None:
            async_update = os.environ.get('TELL_ASYNC_UPDATE', '0') == '1'
        self.async_update = async_update and torch.device(device).type == 'cuda'
        self.update_stream = streams.get('update', device) if self.async_update else None
        self.flat.zero_grad()
        # gradient stores (ops.py): the first eager backward pass is observed, parameters with one dense whole-tensor
        # gradient write per step are then stored by their producer and left alone by BertAdam's zeroing.
        # TELL_GRAD_STORE=0: everything keeps zero + accumulate.
        self._stored_last = False                # the buffer holds gradients that the last update did not zero
        self._store = 'want' if (torch.device(device).type == 'cuda' and
                                 os.environ.get('TELL_GRAD_STORE', '1') != '0') else 'off'
        self.model.register_state_dict_pre_hook(lambda *a, **k: self.finish_update())
        # DP: the gradients of a decoder layer are final when backward leaves the layer (ops.grad_ready_marker); their
        # slice of the flat buffer is handed to RCCL right then (cast to the wire dtype on the backward stream, the
        # collective itself runs on RCCL's stream underneath the rest of backward).  Only what is left (embedder / tied
        # adaptive tables, 35 % of the bytes) is exchanged after backward.
        self._ranges, self._reduced, self._pending, self._in_backward = {}, [], [], False
        self._capturing = False
        # defer_update = True: a step stops after backward - gradients stay in flat.grad (they accumulate over calls
        # until the caller runs optimizer.step(zero_grad=True) or flat.zero_grad()); the captured step graph then ends
        # after backward as well.  Gradient accumulation over micro-batches, and how the parity tests read the
        # gradients a graph REPLAY produced.
        self.defer_update = False
        on_gpu = torch.device(device).type == 'cuda'
        # device-side NaN / Inf skip: [flag, count] read by the optimizer kernel (csrc/optim.hip) - the reference's
        # skip of a NaN batch (:225-227) and apex O2's overflow skip without a host synchronisation
        self.skip = torch.zeros(2, dtype=torch.int32, device=device) if on_gpu else None
        from .step_graph import StepGraph
        self.step_graph = StepGraph(self, capture_after) if on_gpu else None
        self.shape_buckets = tuple(shape_buckets) if shape_buckets else None
        if capture_after is not None and hasattr(model, 'set_capture_after'):
            model.set_capture_after(capture_after)                 # the encoder graphs follow the same policy
        self.bucketed_reduces = 0
        # dp_timing = []: every update then records three events on the update's stream - before the exchange is
        # handed to RCCL, after (casts + collective launches issued), and after the stream has waited for the last
        # bucket; dp_times() turns them into (allreduce_ms, exposed_allreduce_ms) per step
        self.dp_timing = None
        self._test_reduce_scale = None              # tests: emulate world_size 2 with identical ranks (x2 after a reduce)
        # The bucketed exchange needs Python inside backward, i.e. the eager schedule: it is used when the step graph is
        # off (TELL_STEP_GRAPH=0); with the graph the exchange follows backward and hides under the next batch's encoders
        from . import step_graph as _sg
        bucketed_default = '0' if (_sg.ENABLED and on_gpu) else '1'
        if self.dp and on_gpu and os.environ.get('TELL_DP_BUCKETED', bucketed_default) != '0':
            self._ranges = self._layer_ranges()
            if self._ranges:
                rt.set_grad_ready_callback(self._grad_ready)
                self.step_graph = None                   # the exchange is driven from Python inside backward

    def _layer_ranges(self):
        """{prefix: (lo, hi)} - the contiguous slice of the flat buffers that holds exactly the parameters whose name
        starts with 'decoder.layers.<i>.'."""
        fl, out = self.flat, {}
        ends = fl.offsets[1:] + [fl.total]
        for i in range(len(getattr(getattr(self.model, 'decoder', None), 'layers', []))):
            pre = 'decoder.layers.%d.' % i
            idx = [k for k, n in enumerate(fl.names) if n.startswith(pre)]
            if not idx or idx != list(range(idx[0], idx[-1] + 1)):
                return {}                            # not contiguous (tied across layers): keep the single exchange
            out[pre] = (fl.offsets[idx[0]], ends[idx[-1]])
        return out

    def _grad_ready(self, tag):
        """Called from the autograd thread (current stream = the stream backward runs on)."""
        rng_ = self._ranges.get(tag)
        if rng_ is None or not self._in_backward or self._capturing:
            return
        side = ops.flush_wgrad_stream()              # only with the opt-in weight-gradient stream
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        with hip.bound_stream():
            self._start_reduce(*rng_)
        self._reduced.append(rng_)
        self.bucketed_reduces += 1

    def dp_times(self):
        """-> [(allreduce_ms, exposed_allreduce_ms)] of the updates recorded since dp_timing was set (call after a device
        synchronisation).  allreduce_ms: from handing the gradient to RCCL until the update stream holds the reduced
        gradient; exposed: the part of it the update stream spent waiting (nothing of its own left to run) - the
        other streams (the next batch's encoders) keep the GPU busy meanwhile."""
        out = [(e[0].elapsed_time(e[2]), e[1].elapsed_time(e[2])) for e in (self.dp_timing or [])]
        if self.dp_timing is not None:
            self.dp_timing = []
        return out

    def finish_update(self):
        """Make the current stream wait for an in-flight weight update (checkpointing, evaluation, ...)."""
        rt.wait_weight_update()

    def _swap_ema(self):
        f = self.flat
        with hip.bound_stream():
            hip.call('tell_ema_swap', f.flat, f.ema, f.shadow, f.total)
        self.optimizer.ema_swapped = not self.optimizer.ema_swapped
        rt.bump_weights_epoch()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with trainer.ema_weights():` - inside, the model's parameters (state_dict(), forward, generate*,
        score_captions) are the exponential moving average of the weights (optimizer option ema_decay).  One pass
        exchanges the VALUES of the masters and the average and rewrites the bf16 working copy (tell_ema_swap); no
        pointer changes, so every captured graph stays valid exactly as after an optimizer step, and the weights epoch
        is bumped for the caches keyed on it.  The same pass on exit restores all three buffers bit for bit.  No
        training step inside: the masters sit in the EMA buffer."""
        if self.optimizer.ema_decay is None:
            raise ValueError('Trainer.ema_weights() needs the optimizer option ema_decay (got ema_decay=None)')
        if self.optimizer.ema_swapped:
            raise RuntimeError('Trainer.ema_weights() does not nest')
        self.finish_update()
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def ema_state_dict(self):
        """A detached copy of the model's state dict with the averaged weights in place of the trained ones - what to
        save in order to evaluate with them later."""
        with self.ema_weights():
            return {k: v.detach().clone() for k, v in self.model.state_dict().items()}

    def train_one_batch(self, batch, next_batch=None):
        """callback_apex_trainer.py:208-247 for one batch; returns the (detached) loss tensor.

        next_batch: the batch that will be trained next, if the caller already has it (a data loader always
        does).  Its frozen encoders are launched on their own streams BEFORE this batch's decoder work is
        issued, so ResNet-152 / RoBERTa-large of step N+1 fill the GPU underneath the latency-bound decoder
        forward, backward and optimizer of step N.  Numerics are unchanged: the encoders read no trainable
        weight, and BatchNorm running statistics are still updated in batch order on the encoder stream."""
        if self.optimizer.ema_swapped:
            raise RuntimeError('train_one_batch inside Trainer.ema_weights(): the masters sit in the EMA buffer')
        # (only with a next batch to encode underneath: alone the narrow launches are 1.3x slower and nothing fills the
        #  CUs they leave - the decoder step alone 6.87 -> 7.48 ms)
        overlapped = bool(self._lib_options) and next_batch is not None
        scoped = hip.options(**self._lib_options) if overlapped else contextlib.nullcontext()
        with hip.bound_stream(), scoped:
            return self._train_one_batch(batch, next_batch)

    def _encoded_for(self, batch):
        pre, self._prefetched = getattr(self, '_prefetched', None), None
        if pre is not None and pre[0] is batch.get('image') and not pre[1].stale():
            return pre[1]           # (stale: other encode() / generate() calls in between reused the graph's buffers)
        return None

    def _bucketed(self, batch):
        """The batch padded to the shape buckets (see __init__); a batch that already fits is returned as it is."""
        from . import step_graph as _sg
        from .. import graphs
        if self.shape_buckets is None or not (_sg.ENABLED and graphs.ENABLED) or self.nan_check:
            return batch
        if not getattr(self.model, 'SHAPE_BUCKETS', True):     # a model whose loss sees the padding (models/pointer.py)
            return batch
        idx = getattr(self.model, 'index', 'roberta')
        pad = int(getattr(self.model, 'padding_idx', 1))
        out = None

        def grow(t, dim, n, value):
            shape = list(t.shape)
            shape[dim] = n - t.shape[dim]
            return torch.cat([t, t.new_full(shape, value)], dim=dim)
        # a caption of T + 1 tokens makes T decoder positions: T is what gets bucketed
        for key, mult, extra in (('context', self.shape_buckets[0], 0), ('caption', self.shape_buckets[1], 1)):
            field = batch.get(key)
            ids = field.get(idx) if isinstance(field, dict) else None
            if not (torch.is_tensor(ids) and ids.is_cuda and ids.dim() == 2):
                continue
            n = -(-(ids.shape[1] - extra) // mult) * mult + extra
            if n != ids.shape[1]:
                out = dict(batch) if out is None else out
                f = dict(field)
                f[idx] = grow(ids, 1, n, pad)
                for mk in (idx + '_copy_masks', idx + '_proper_masks'):      # masks are padded with -1
                    m = f.get(mk)
                    if torch.is_tensor(m) and m.dim() == 2 and m.shape[1] == ids.shape[1]:
                        f[mk] = grow(m, 1, n, -1)
                out[key] = f
        for key, rows in (('face_embeds', 4), ('obj_embeds', 64)):
            t = batch.get(key)
            if torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.shape[2] > 0 and t.shape[1] < rows:
                out = dict(batch) if out is None else out
                out[key] = grow(t, 1, rows, float('nan'))
        return batch if out is None else out

    @staticmethod
    def _store_safe(batch):
        """Store mode rests on every marked tensor being rewritten WHOLE by this step's backward pass.  The one
        data-dependent exception: a batch in which no sample has a face / an object hands the model an EMPTY context
        ([B,1,0], collate's empty field), for which the K / V projections of that context are skipped (blocks.py
        kv_project_all, modules/attention.py project_kv; multi_head.py:349-374) - rows [E,3E) of its in_proj_weight
        then get no gradient write, and a stored buffer would still hold the previous step's rows.  Such a step runs
        with the zero + accumulate convention (shape test on the host: no synchronisation)."""
        for key in ('face_embeds', 'obj_embeds'):
            t = batch.get(key) if isinstance(batch, dict) else None
            if torch.is_tensor(t) and t.dim() == 3 and (t.shape[1] == 0 or t.shape[2] == 0):
                return False
        return True

    def _grad_store_begin(self, batch=None):
        """Select this step's gradient convention.  Store mode needs an update after every backward pass (micro-batch
        accumulation - defer_update - adds into the buffer) and a batch whose backward pass writes every marked tensor
        (_store_safe); leaving it, the stored gradients of the last step are still in the buffer and have to go.  While
        the buffer holds accumulated gradients that no update has consumed yet (a defer_update pass came before), the
        pass that ends the accumulation must ADD to them too: store mode stays off until an update / zero_grad has
        cleared the buffer (flat.accum_pending)."""
        want = (self._store == 'ready' and not self.defer_update and not self.flat.accum_pending and
                (batch is None or self._store_safe(batch)))
        if self._stored_last and not want:       # (this trainer's own history: the switch in ops.py is process-wide)
            pending = self.flat.accum_pending
            self.flat.zero_grad()
            self.flat.accum_pending = pending
        self._stored_last = want
        ops.grad_store_mode(want)
        if self.defer_update:
            self.flat.accum_pending = True

    def _train_one_batch(self, batch, next_batch=None):
        try:
            return self._train_one_batch_body(batch, next_batch)
        finally:
            ops.grad_store_mode(False)           # outside a trainer step every backward pass accumulates

    def _train_one_batch_body(self, batch, next_batch=None):
        if not self.model.training:              # (recursing through ~650 modules costs 2.5 ms of host time)
            self.model.train()                   # (:214 zero_grad: done right after the previous update)
        batch = self._bucketed(batch)
        self._grad_store_begin(batch)
        if next_batch is not None:
            next_batch = self._bucketed(next_batch)
        enc = None
        if hasattr(self.model, 'encode') and torch.is_tensor(batch.get('image')) and batch['image'].is_cuda:
            enc = self._encoded_for(batch)
            if enc is None:
                enc = self.model.encode(batch['context'], batch['image'])
            if next_batch is not None:
                self._prefetched = (next_batch['image'],
                                    self.model.encode(next_batch['context'], next_batch['image'], ahead=True))
        loss = None
        if enc is not None and self.step_graph is not None and not self.nan_check:
            loss = self.step_graph.run(batch, enc, self._eager_step)      # decoder fwd + loss + bwd (+ update) replayed
        if loss is None:
            loss = self._eager_step(batch, enc)
        if loss is not None:
            self.batch_num_total += 1
        return loss

    def _flag_loss(self, loss):
        """skip[0] = the loss is NaN / Inf (:225-227 skips such a batch; here the optimizer kernel does, no host sync)."""
        if loss.is_cuda:
            hip.call('tell_loss_flag', loss.detach().reshape(1).float(), self.skip)

    def _backward(self, scaled):
        self._in_backward = True
        # the weight-norm chain rule of all GehringLinears runs as ONE launch after the pass - unless gradient buckets
        # leave during backward (a layer's gradients have to be final at its marker then)
        ops.wn_defer(not self._ranges)
        ops.wgrad_group_defer(not self._ranges)                          # ... and so do the weight-gradient GEMMs
        ops.finish_defer(not self._ranges)                               # ... and the small column-sum finishers
        observe = self._store == 'want' and not self._capturing
        if observe:
            ops.grad_store_observe(True)
        try:
            scaled.backward()                                            # :229-231
        except BaseException:
            ops.wn_drop()
            ops.wgrad_group_drop()
            ops.finish_drop()
            if observe:
                ops.grad_store_observe(False)
            raise
        finally:
            self._in_backward = False
            ops.wn_defer(False)
            ops.wgrad_group_defer(False)
            ops.finish_defer(False)
        ops.join_wgrad_stream()                                          # weight-gradient side stream (ops.py)
        ops.wgrad_group_flush()
        ops.wn_flush()
        ops.finish_flush()
        if observe:
            # the gradients in the buffer are complete and were accumulated onto zeros: the convention can change right
            # here - this step's update already leaves the marked tensors alone, the next pass stores over them.  (Every
            # graph is captured after this point: the convention a signature is captured with follows from defer_update,
            # which is part of the signature.)
            self.flat.set_grad_store(ops.grad_store_observe(False))
            self._store = 'ready'
            self._stored_last = not self.defer_update
            ops.grad_store_mode(self._stored_last)

    def skipped_steps(self):
        """Number of optimisation steps the device-side NaN / Inf check turned into no-ops so far (one host sync)."""
        return int(self.skip[1].item()) if self.skip is not None else 0

    def _eager_step(self, batch, enc=None):
        extra = {'encoded': enc} if enc is not None else {}
        return self._finish_step(self.model(**batch, **extra))           # :220 / :194

    def _finish_step(self, out):
        """Everything of the eager step behind the model's forward pass: NaN flag, backward, exchange and update."""
        loss = out['loss']
        if loss is None:             # the pointer models' batches without a copy target: no backward, no update
            return None
        self._flag_loss(loss)
        n_local = None
        if self.dp and self._ranges:
            # bucketed exchange during backward: the per-rank weight has to be in the gradients before the first
            # bucket leaves, i.e. on the loss
            scaled = loss * dp.loss_weight(out['sample_size'].to(torch.float32).reshape(1), self.dist,
                                           self.world).reshape(())
        else:
            scaled = loss
            n_local = out['sample_size'] if self.dp else None
        if self.nan_check:                                               # :225-227 with the reference's host sync
            bad = (~torch.isfinite(loss.detach())).to(torch.float32)
            if self.dp:
                self.dist.all_reduce(bad)
            if bad.item() > 0:
                self.flat.zero_grad()
                return None
        self._backward(scaled)
        if self.async_update:
            main = torch.cuda.current_stream()
            self.update_stream.wait_stream(main)
            with torch.cuda.stream(self.update_stream), hip.bound_stream():
                self._update(n_local)
                done = torch.cuda.Event()
                done.record(self.update_stream)
            rt.set_pending_update(done)
        else:
            self._update(n_local)
        return loss.detach()

    # ---- self-critical sequence training --------------------------------------------------
    SCST_BASELINES = ('leave_one_out', 'greedy')

    @staticmethod
    def check_self_critical(n_samples=4, baseline='leave_one_out', max_order=4, reward=None):
        """The arguments of train_self_critical / the trainer key `self_critical` -> (n, baseline, max_order)."""
        n, k = n_samples, max_order
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 16:
            raise ValueError('self_critical: n_samples must be an integer in 1..16 (got %r)' % (n,))
        if baseline not in Trainer.SCST_BASELINES:
            raise ValueError("self_critical: baseline must be 'leave_one_out' or 'greedy' (got %r)" % (baseline,))
        if baseline == 'leave_one_out' and n == 1:
            raise ValueError("self_critical: baseline='leave_one_out' needs n_samples >= 2 (one sample has no others)")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 4:
            raise ValueError('self_critical: max_order must be an integer in 1..4 (got %r)' % (k,))
        if reward is not None and not callable(reward):
            raise ValueError('self_critical: reward must be callable(gen_ids_samples, batch) -> fp32 [B, n] or None')
        return n, baseline, k

    def train_self_critical(self, batch, n_samples=4, baseline='leave_one_out', max_order=4, reward=None):
        """One self-critical step: n_samples captions per image are drawn from ONE pass of the encoders
        (generate(n_samples=n, rank_by='draw'), eval mode, no_grad), scored against batch['caption'] on the device
        (tell_caption_reward: sentence-level GLEU over the n-gram orders 1..max_order) and reinforced by the weighted
        training pass forward(per_image=n, caption_weights=adv) through the tail of the plain step (_flag_loss, _backward,
        _update).  baseline: 'leave_one_out' (the mean reward of the image's other samples) or 'greedy' (the reward of one
        more, arg-max, generate).  reward = callable(gen_ids_samples [B, n, L], batch) -> fp32 [B, n] replaces the kernel's
        reward; the advantage then follows the same definition in torch.  The step is never captured and runs under the
        zero + accumulate gradient convention, whichever the plain step uses; it leaves that choice as it found it.
        -> {'loss' (sum_r adv_r sum_t -log p(y_rt) over the sampled tokens, bits per token), 'reward_mean',
        'baseline_mean', 'reward' [B, n], 'adv' [B, n], 'baseline' ([B, 1] greedy: what the kernel subtracted; [B, n]
        leave-one-out: reward - adv), 'gen_ids_samples' [B, n, L] (the captions the rewards belong to)}, all device tensors."""
        n, baseline, max_order = self.check_self_critical(n_samples, baseline, max_order, reward)
        sampling = getattr(self.model, '_sampling', None)
        if not callable(sampling) or sampling() is None:
            raise ValueError('train_self_critical needs a sampling model (sampling_topk > 1, sampling_topp, sampling_minp '
                             'or sampling_typical): %s decodes by arg-max' % type(self.model).__name__)
        if self.optimizer.ema_swapped:
            raise RuntimeError('train_self_critical inside Trainer.ema_weights(): the masters sit in the EMA buffer')
        store, self._store = self._store, 'off'      # no store mode and no observing pass here (_grad_store_begin, _backward)
        try:
            return self._self_critical_body(batch, n, baseline, max_order, reward)
        finally:
            self._store = store
            ops.grad_store_mode(False)

    @contextlib.contextmanager
    def _arg_max_decode(self):
        """Inside, the sampling model decodes by arg-max (the greedy baseline caption)."""
        m = self.model
        keys = ('sampling_topk', 'sampling_topp', 'sampling_minp', 'sampling_typical')
        saved = {k: getattr(m, k, None) for k in keys}
        m.sampling_topk, m.sampling_topp, m.sampling_minp, m.sampling_typical = 1, None, None, None
        try:
            yield
        finally:
            for k, v in saved.items():
                setattr(m, k, v)

    def _self_critical_body(self, batch, n, baseline, max_order, reward_fn):
        model = self.model
        idx = model.index
        pad, eos = int(model.padding_idx), 2
        if not model.training:
            model.train()                            # the encoders run as they do for the plain step
        batch = self._bucketed(batch)
        self._grad_store_begin(batch)
        fields = {k: batch[k] for k in ('context', 'image', 'caption', 'face_embeds', 'obj_embeds') if k in batch}

        def fresh():                                 # (_forward rewrites caption[index]: never the caller's dict)
            return {k: (dict(v) if isinstance(v, dict) else v) for k, v in fields.items()}
        enc = self._encoded_for(batch)
        if enc is None:
            with hip.bound_stream():
                enc = model.encode(batch['context'], batch['image'])
        ref = batch['caption'][idx][:, :257]         # (the reward reads at most 256 reference tokens behind <s>)
        B = ref.shape[0]
        model.eval()
        try:
            with torch.no_grad():
                gen = model.generate(**fresh(), encoded=enc, n_samples=n, rank_by='draw')
                samples = gen['gen_ids_samples'] if n > 1 else gen['gen_ids'].unsqueeze(1)       # [B, n, L]
                greedy = None
                if baseline == 'greedy':
                    with self._arg_max_decode():
                        greedy = model.generate(**fresh(), encoded=enc)['gen_ids']
        finally:
            model.train()
        with torch.no_grad(), hip.bound_stream():
            reward, adv, base = self._caption_rewards(samples, greedy, ref, batch, pad, eos, max_order, reward_fn)
            # the training captions: <s>, the sample up to and with its </s>; what lies behind a drawn pad id is not a
            # target (the reward stops there too)
            cap = samples.reshape(B * n, -1).clone()
            lead = (cap[:, 1:] != pad).long().cumprod(1).bool()
            cap[:, 1:] = torch.where(lead, cap[:, 1:], torch.full_like(cap[:, 1:], pad))
        train = fresh()
        train['caption'] = {idx: cap}
        with hip.bound_stream():
            if enc.stale():                          # a generate that encoded on its own has reused the buffers
                enc = model.encode(batch['context'], batch['image'])
            out = model(**train, encoded=enc, per_image=n, caption_weights=adv.reshape(B * n))
            loss = self._finish_step(out)
        if loss is None:                             # (nan_check=True: the host-synchronous skip of the plain step)
            return None
        self.batch_num_total += 1
        return {'loss': loss, 'reward_mean': reward.mean(), 'baseline_mean': base.mean(), 'reward': reward,
                'adv': adv, 'baseline': base, 'gen_ids_samples': samples}

    def _caption_rewards(self, samples, greedy, ref, batch, pad, eos, max_order, reward_fn):
        """-> (reward [B, n], adv [B, n], baseline [B, 1] (greedy) or [B, n]) of samples int64 [B, n, L] against ref int64 [B, T]."""
        from ..models.transformer import caption_reward_definition
        B, n, L = samples.shape
        ids = samples.reshape(B * n, L).contiguous()

        def kernel(h, per, baseline=None):           # the launch on the device, its numpy definition on the CPU
            if h.is_cuda:
                return ops.caption_reward(h, ref, B, per, h.shape[1] - 1, ref.shape[1] - 1, pad, eos, max_order,
                                          baseline=baseline)[:2]
            d = caption_reward_definition(h.numpy(), ref.numpy(), per, h.shape[1] - 1, ref.shape[1] - 1, pad, eos, max_order,
                                          None if baseline is None else baseline.numpy())
            return torch.from_numpy(d['reward']), torch.from_numpy(d['adv'])
        base = None
        if greedy is not None:
            base = (reward_fn(greedy.unsqueeze(1), batch).reshape(B) if reward_fn is not None
                    else kernel(greedy.contiguous(), 1)[0].reshape(B)).float().contiguous()
        if reward_fn is None:
            reward, adv = kernel(ids, n, base)
        else:
            reward = reward_fn(samples, batch)
            if not torch.is_tensor(reward) or reward.dtype != torch.float32 or tuple(reward.shape) != (B, n):
                raise ValueError('self_critical: reward(gen_ids_samples, batch) must return fp32 [%d, %d]' % (B, n))
            if base is not None:
                adv = reward - base.unsqueeze(1)
            elif n > 1:
                # leave-one-out by tell_caption_reward's definition: the others in ascending j, one fp32 accumulator
                s = torch.zeros_like(reward)
                for e in range(n):
                    others = torch.ones(n, dtype=torch.bool, device=reward.device)
                    others[e] = False
                    s = torch.where(others, s + reward[:, e:e + 1], s)
                adv = reward - s / float(n - 1)
            else:
                adv = reward.clone()
        return reward, adv, (reward - adv if base is None else base.unsqueeze(1))

    def _update(self, n_local=None):
        """Gradient exchange (data parallel) + BertAdam + gradient zeroing.  n_local: this rank's token count when
        the loss was NOT weighted before backward (graph replay, unbucketed eager): the weight n_local * world /
        n_global is then applied to the gradient on its way to the wire."""
        if self.defer_update:
            return
        if self.dp:
            scale = None
            ev = None
            if self.dp_timing is not None and self.flat.grad.is_cuda:      # bench / diagnosis: events, read after a sync
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
            if n_local is not None:
                scale = dp.loss_weight(n_local.to(torch.float32).reshape(1), self.dist, self.world)
            if self.skip is not None and self.skip.is_cuda:
                self.dist.all_reduce(self.skip[:1], op=self.dist.ReduceOp.MAX)        # collective NaN skip
            done, self._reduced = sorted(self._reduced), []
            lo = 0
            for a, b in done + [(self.flat.total, self.flat.total)]:     # everything not exchanged during backward
                if a > lo:
                    self._start_reduce(lo, a, scale)
                lo = max(lo, b)
            if ev is not None:
                ev[1].record()
            wire = self._finish_reduces()
            if ev is not None:
                ev[2].record()
                self.dp_timing.append(ev)
            if wire is not None:                       # bf16 on the wire: BertAdam reads the reduced buffer as it is
                self.optimizer.step(grad_scale=1.0 / self.world, zero_grad=True, skip=self.skip, grad_wire=wire)
                return
        self.optimizer.step(grad_scale=1.0 / self.world, zero_grad=True, skip=self.skip)  # :238 (+ :214 of the next batch)

    def _cast(self, src, dst):
        hip.call('tell_cast', src, hip.dt(src), dst, hip.dt(dst), src.numel())

    def _start_reduce(self, lo, hi, scale=None):
        """Hand flat.grad[lo:hi] to RCCL (asynchronously; bf16 on the wire in bf16 mode, see dp.all_reduce_flat_bf16).
        scale: optional device scalar multiplied in on the way (the rank's loss weight)."""
        grad = self.flat.grad[lo:hi]
        if self.allreduce_dtype == torch.bfloat16:
            if self._wire is None:
                self._wire = torch.empty(self.flat.total, dtype=torch.bfloat16, device=self.flat.grad.device)
            buf, step = self._wire[lo:hi], 2 * self.bucket_elems
            hip.call('tell_scale_cast', grad, buf, hip.BF16, grad.numel(), scale)
        else:
            buf, step = grad, self.bucket_elems
            if scale is not None:
                if grad.is_cuda:
                    hip.call('tell_scale_cast', grad, grad, hip.F32, grad.numel(), scale)
                else:
                    grad.mul_(scale)
        handles = [self.dist.all_reduce(buf[s:s + step], async_op=True) for s in range(0, buf.numel(), step)]
        self._pending.append((lo, hi, handles))

    def _finish_reduces(self):
        """The current stream waits for every exchange in flight.  -> the bf16 wire buffer when it now holds the WHOLE
        reduced gradient and the optimizer kernel can read it directly (CUDA, bf16 on the wire, one exchange covering
        all of flat.grad), else None after widening the bf16 results back into flat.grad."""
        pending, self._pending = self._pending, []
        for lo, hi, handles in pending:
            for h in handles:
                h.wait()
        direct = (self.allreduce_dtype == torch.bfloat16 and self._test_reduce_scale is None and
                  self.flat.grad.is_cuda and len(pending) == 1 and pending[0][0] == 0 and
                  pending[0][1] == self.flat.total and hasattr(self.optimizer, 'launch'))
        if direct:
            return self._wire
        for lo, hi, handles in pending:
            grad = self.flat.grad[lo:hi]
            if self.allreduce_dtype == torch.bfloat16:
                self._cast(self._wire[lo:hi], grad)
            if self._test_reduce_scale is not None:
                grad.mul_(self._test_reduce_scale)
        return None


@TrainerBase.register('callback_apex')
class CallbackApexTrainer(Trainer):
    """Registration name of the reference trainer (callback_apex_trainer.py:51).  The AllenNLP
    callback machinery (checkpoint / tensorboard / validation callbacks) is out of scope;
    `apex_opt_level` / `keep_batchnorm_fp32` are accepted and ignored (bf16 + fp32 masters)."""

    def __init__(self, model, optimizer=None, no_grad=(r'^resnet', r'^roberta'), apex_opt_level=None,
                 keep_batchnorm_fp32=None, num_epochs=1, shuffle=True, cuda_device=0, callbacks=None, self_critical=None,
                 **kw):
        """self_critical: {n_samples, baseline, max_order} - `train` then runs Trainer.train_self_critical on every batch
        (the second training stage); absent: the plain step."""
        super().__init__(model, optimizer, no_grad, device='cuda' if cuda_device is not None else 'cpu')
        self.num_epochs = num_epochs
        self.self_critical = None
        if self_critical is not None:
            extra = set(self_critical) - {'n_samples', 'baseline', 'max_order'}
            if extra:
                raise ValueError('self_critical: unknown keys %s (n_samples, baseline, max_order)' % sorted(extra))
            n, base, k = self.check_self_critical(**self_critical)
            self.self_critical = {'n_samples': n, 'baseline': base, 'max_order': k}

    def train(self, batches):
        losses = []
        for batch in batches:
            if self.self_critical is not None:
                losses.append(self.train_self_critical(batch, **self.self_critical)['loss'])
            else:
                losses.append(self.train_one_batch(batch))
        return losses
