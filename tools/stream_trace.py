#!/usr/bin/env python3
"""The order of every launch and every stream wait of a training step, as text: run it on two trees and compare the outputs line by line.

`hip_ops.call` is replaced by a recorder (it notes the entry point and the stream it is queued on, then calls through), and
`torch.cuda.Stream.wait_stream`, `Stream.wait_event` and `Event.record` are wrapped.  Streams are labelled s0, s1, ... in the order they
first appear, so the text does not depend on handles.  Per step, in program order:
    launch <entry point> <stream>
    wait   <waiter> <- <waited-for>        (wait_stream; wait_event names the stream the event was recorded on)
    record <stream>
for two consecutive steps, optimizer included, of: ecamp_tiny, bf16, B = 4, S = 64 (per-layer weight gradients); ecamp(), bf16, B = 8,
S = 128 (rows = 400: the grouped launch qualifies); ECAMPClassifier(train_encoder=True) on ecamp_tiny, bf16, B = 8.
usage: stream_trace.py > trace.txt"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ecamp_amd import engine_finetune, hip_ops, optim
from ecamp_amd.data import synthetic_batch
from ecamp_amd.module import model_ecamp
from ecamp_amd.module.classifier import ECAMPClassifier
from ecamp_amd.util.misc import NativeScalerWithGradNormCount

lines, labels = [], {}


def label(st):
    return labels.setdefault(st.cuda_stream, "s%d" % len(labels))


def install():
    call = hip_ops.call
    wait_stream, wait_event, record = torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record

    def traced_call(name, *args):
        lines.append("launch %s %s" % (name, label(torch.cuda.current_stream())))
        return call(name, *args)

    def traced_wait_stream(self, other):
        lines.append("wait   %s <- %s" % (label(self), label(other)))
        return wait_stream(self, other)

    def traced_wait_event(self, event):
        lines.append("wait   %s <- %s (event)" % (label(self), getattr(event, "_traced_on", "?")))
        return wait_event(self, event)

    def traced_record(self, stream=None):
        stream = torch.cuda.current_stream() if stream is None else stream
        self._traced_on = label(stream)
        lines.append("record %s" % self._traced_on)
        return record(self, stream)

    hip_ops.call = traced_call
    torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = traced_wait_stream, traced_wait_event, traced_record


def flush(title):
    print("== %s: %d lines" % (title, len(lines)))
    print("\n".join(lines))
    del lines[:]


def pretrain(title, model, B, S, dev):
    model = model.to(dev)
    model.train()
    opt = optim.FusedAdamW(optim.add_weight_decay(model, 0.05), lr=1.5e-4, betas=(0.9, 0.95))
    scaler = NativeScalerWithGradNormCount()
    batch = synthetic_batch(B, S, 448, seed=0, device=dev)
    del lines[:]   # (building the model and the batch is not a step)
    for step in range(2):
        scaler(sum(model(batch)), opt, parameters=model.parameters(), update_grad=True)
        opt.zero_grad()
        flush("%s step %d" % (title, step))
    torch.cuda.synchronize()


def finetune(title, B, dev):
    enc = model_ecamp.ecamp_tiny(compute_dtype=torch.bfloat16)
    clf = ECAMPClassifier(enc, 5, multilabel=True, train_encoder=True).to(dev)
    args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=1, num_steps=2, max_grad_norm=1.0)
    opt = engine_finetune.make_optimizer(clf, args)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    y = (torch.rand(B, 5, generator=g) < 0.5).float().to(dev)
    del lines[:]
    for step in range(2):
        engine_finetune.train_step(clf, opt, x, y, step, args)
        flush("%s step %d" % (title, step))
    torch.cuda.synchronize()


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    install()
    pretrain("ecamp_tiny bf16 B=4 S=64", model_ecamp.ecamp_tiny(compute_dtype=torch.bfloat16), 4, 64, dev)
    pretrain("ecamp bf16 B=8 S=128", model_ecamp.ecamp(compute_dtype=torch.bfloat16), 8, 128, dev)
    finetune("ECAMPClassifier(train_encoder=True) on ecamp_tiny bf16 B=8", 8, dev)
    print("== streams: %d" % len(labels))


if __name__ == "__main__":
    main()
