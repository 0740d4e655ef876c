"""Inference forward -- drop-in for reference src/test.py:16-50 (`test(args, encoder, decoder, x)`).

Eval-mode encoder once, decoder T = args.maxseqlen steps, masks resized to the input size, returns
(sigmoid(masks) [B,T,H,W], class probabilities [B,T,C], sigmoid(stop) [B,T,1]).  Runs under torch.no_grad()
(the reference pre-dates it and relied on volatile Variables); `return_logits=True` returns the raw mask / stop logits.
"""
import torch

from . import ops


@torch.no_grad()
def test(args, encoder, decoder, x, return_logits=False):
    T = args.maxseqlen
    hidden = None
    out_masks, out_classes, out_stops = [], [], []
    encoder.eval()
    decoder.eval()
    # (under -dtype bf16 with the decoder on blk storage the encoder hands its skip features over as blk tensors, as in runIter: no fp32
    #  NCHW copies between trunk, skip branches and decoder)
    from . import train as _train
    blk_ok = (x.is_cuda and _train.BLK_SKIPS[0] and hasattr(encoder, "sk5") and hasattr(decoder, "clstm_list") and
              "forward" not in encoder.__dict__ and hasattr(decoder, "forward_sequence") and _train._blk_skips_ok(encoder, decoder, x, T))
    feats = encoder(x, blk_skips=True) if blk_ok else encoder(x)        # test.py:35
    if any(f.dim() == 5 for f in feats):
        from . import blk_trunk, decoder_seq
        if not decoder_seq.supported(decoder, feats, T):                # (same predicate as blk_ok asked: a conversion, never a crash)
            feats = [blk_trunk.to_nchw(f) if f.dim() == 5 else f for f in feats]
    steps, hidden = decoder.forward_sequence(feats, T)                  # test.py:37-38 (the T decoder steps, wavefront order)
    for out_mask, out_class, out_stop in steps:
        out_mask = ops.upsample_bilinear_ac(out_mask, (x.size()[-2], x.size()[-1]))   # test.py:39-40
        out_masks.append(out_mask)
        if out_class.dim() == 1:       # a batch of one on the per-step path: RSIS.forward keeps the reference's 1-D (C,) / (1,) outputs
            out_class, out_stop = out_class.view(1, -1), out_stop.view(1, -1)
        out_classes.append(out_class)
        out_stops.append(out_stop)
    out_masks = torch.cat(out_masks, 1)                                 # test.py:46
    out_classes = torch.cat(out_classes, 1).view(out_class.size(0), len(out_classes), -1)   # test.py:47
    out_stops = torch.cat(out_stops, 1).view(out_stop.size(0), len(out_stops), -1)          # test.py:48
    if return_logits:
        return out_masks, out_classes, out_stops
    return torch.sigmoid(out_masks), out_classes, torch.sigmoid(out_stops)                   # test.py:50


class GraphedTest(object):
    """test() captured ONCE per input shape as a hipGraph and replayed: the ~560 kernel launches of an inference batch cost the
    host as long in Python (12 ms at batch 32, T = 10) as the GPU needs for them.  The first `warm` calls run eagerly (they load
    code objects and let BatchNorm / packed-weight caches settle), the next one captures; the input is copied into a static buffer
    and the returned tensors are STATIC -- the next call overwrites them, so consume (or clone) them first.  A new input shape re-captures.
    So does a change of the weights: the packed copies are part of the captured launches' arguments, so the capture records a weights key
    (the packed-weight epoch, which the optimizer steps and the replays of a captured training step bump, and every parameter's
    (_version, data_ptr()), which load_state_dict and other in-place writes bump); a call that finds another key runs test() eagerly
    (which repacks the copies from the live weights) and the next call captures again.  Writes through `.data` bypass `_version`: after
    one, call ops.bump_weight_epoch()."""

    def __init__(self, args, encoder, decoder, return_logits=False, warm=2):
        self.args, self.encoder, self.decoder, self.return_logits, self.warm = args, encoder, decoder, return_logits, warm
        self.graph, self.static_x, self.outs, self.n_eager = None, None, None, 0
        self.params, self.key = None, None
        self.stream = torch.cuda.Stream()

    def _weights_key(self):
        return (ops._WEIGHT_EPOCH[0],) + tuple((p._version, p.data_ptr()) for p in self.params)

    def __call__(self, x):
        if self.graph is not None and self._weights_key() != self.key:
            self.graph, self.static_x, self.outs, self.n_eager = None, None, None, self.warm - 1  # new weights: repack eagerly, capture again
        if self.graph is not None and tuple(x.shape) != tuple(self.static_x.shape):
            self.graph, self.static_x, self.outs, self.n_eager = None, None, None, self.warm      # new shape: capture again
        if self.graph is None:
            if self.n_eager < self.warm:
                self.n_eager += 1
                return test(self.args, self.encoder, self.decoder, x, self.return_logits)
            self.static_x = x.clone()
            torch.cuda.synchronize()
            # (the parameter list is taken once per capture: walking the module tree on every call costs 0.5 ms of host time)
            self.params = list(self.encoder.parameters()) + list(self.decoder.parameters())
            self.key = self._weights_key()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
                self.outs = test(self.args, self.encoder, self.decoder, self.static_x, self.return_logits)
            self.graph = g
        if x.data_ptr() != self.static_x.data_ptr():
            self.static_x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.outs
