"""Generate the fixtures that stand in for the reference checkout in the CPU tests (run where the reference is).

    python oracle/make_golden_reference_files.py <reference checkout>

  tests/golden/test_dataset_masked.pkl           the reference's tests/test_dataset.pkl, byte for byte except payloads:
                                                 patient identifiers -> same-length anonymous tokens, and every payload
                                                 of the clinical cohort frame / processed file list blanked (nothing
                                                 the ingest reads).  Same opcodes, same lengths, same windows.
  tests/golden/ref_checkpoint_resnet18_{zip,legacy}.pth.gz
                                                 whole CNNLinearNetwork(resnet18) modules pickled by the REAL reference
                                                 classes (no class source text stored), every tensor a per-key pattern
                                                 (compressible; ref_checkpoint_pattern() in the test restates it)
  tests/golden/ref_checkpoint_resnet18.json      the reference module's state_dict keys, in order
  tests/golden/ref_import_logits.npz             the reference CNNLinearNetwork's train-mode logits on the first
                                                 golden batch (seeded_params(backbone, 5)), resnet18 and densenet18

Nothing from the reference is copied: the fixtures hold data and recorded outputs only.
"""
import glob
import gzip
import io
import json
import os
import pickletools
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

_STRINGS = ('SHORT_BINSTRING', 'BINSTRING', 'SHORT_BINUNICODE', 'BINUNICODE', 'SHORT_BINBYTES', 'BINBYTES')
_NUMBERS = {'BINFLOAT': 8, 'BININT': 4, 'BININT1': 1, 'BININT2': 2}
_MASKED_KEYS = (b'cohort', b'processed_files')


def _string_payload(data, pos, op):
    """(start, length) of the payload bytes of string opcode `op` at `pos`."""
    width = 1 if op.name.startswith('SHORT_') else 4
    n = int.from_bytes(data[pos + 1:pos + 1 + width], 'little')
    return pos + 1 + width, n


def mask_dataset_pickle(src):
    data = bytearray(open(src, 'rb').read())
    ops = list(pickletools.genops(io.BytesIO(bytes(data))))
    # replay the stack with, for every entry, the first opcode that built it; a SETITEM(S) then tells which opcodes
    # built the value of each key it stores
    stack, marks, masked = [], [], []
    for i, (op, arg, pos) in enumerate(ops):
        if op.name == 'MARK':
            marks.append(len(stack))
            continue
        before = op.stack_before
        if pickletools.markobject in before:
            m = marks.pop()
            below = before.index(pickletools.markobject)
            popped, sliced = stack[m - below:], stack[m:]
            del stack[m - below:]
        else:
            popped, sliced = stack[len(stack) - len(before):], []
            del stack[len(stack) - len(before):]
        if op.name in ('SETITEMS', 'SETITEM'):
            pairs = sliced if op.name == 'SETITEMS' else popped[1:]
            for k in range(0, len(pairs), 2):
                if pairs[k][1] in _MASKED_KEYS:
                    end = pairs[k + 2][0] if k + 2 < len(pairs) else i
                    masked.append((pairs[k + 1][0], end))
        start = min([e[0] for e in popped] + [i])
        key = None
        if op.name in _STRINGS and isinstance(arg, (bytes, str)):
            key = arg.encode('latin-1') if isinstance(arg, str) else arg
        stack.extend([(start, key)] * len(op.stack_after))
    assert len(masked) == len(_MASKED_KEYS), masked
    for lo, hi in masked:
        for op, arg, pos in ops[lo:hi]:
            if op.name in _STRINGS:
                s, n = _string_payload(data, pos, op)
                data[s:s + n] = b'x' * n
            elif op.name in _NUMBERS:
                data[pos + 1:pos + 1 + _NUMBERS[op.name]] = b'\0' * _NUMBERS[op.name]
    ids = sorted({m.group(0) for m in re.finditer(rb'[0-9A-Za-z*]*RPI[0-9*]+', bytes(data))})
    for k, pid in enumerate(ids):
        tok = b'P' + str(k).encode().rjust(len(pid) - 1, b'0')
        data = bytearray(bytes(data).replace(pid, tok))
    assert b'RPI' not in data
    return bytes(data)


def ref_checkpoint_pattern(state_dict):
    """Every entry of a state_dict set to a pattern of its key index (the test restates this)."""
    with torch.no_grad():
        for i, (k, v) in enumerate(state_dict.items()):
            if v.dtype.is_floating_point:
                pat = (torch.arange(v.numel(), dtype=torch.float64) % 7) * 0.125 + (i + 1) * 0.01
                v.copy_(pat.view(v.shape))
            else:
                v.fill_(i)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from deepards.models.resnet import resnet18
    from deepards.models.densenet import densenet18
    from deepards.models.torch_cnn_linear_network import CNNLinearNetwork
    from oracle import torch_ref
    from oracle.weights import seeded_params

    masked = mask_dataset_pickle(os.path.join(ref_root, 'deepards', 'tests', 'test_dataset.pkl'))
    open(os.path.join(OUT, 'test_dataset_masked.pkl'), 'wb').write(masked)

    import torch.serialization as S

    def no_source(obj):
        raise OSError('class source text is not stored in the fixture')
    S.get_source_lines_and_file = no_source
    torch.manual_seed(0)
    ref = CNNLinearNetwork(resnet18(), 20, 0)
    ref_checkpoint_pattern(ref.state_dict())
    for tag, legacy in (('zip', False), ('legacy', True)):
        buf = io.BytesIO()
        torch.save(ref, buf, _use_new_zipfile_serialization=not legacy)
        with gzip.GzipFile(os.path.join(OUT, 'ref_checkpoint_resnet18_%s.pth.gz' % tag), 'wb', mtime=0) as f:
            f.write(buf.getvalue())
    json.dump(list(ref.state_dict()), open(os.path.join(OUT, 'ref_checkpoint_resnet18.json'), 'w'), indent=0)

    gold = sorted(p for p in glob.glob(os.path.join(OUT, '*net18_*.npz'))
                  if not os.path.basename(p).startswith(('head_', 'opt_')))
    x = torch.from_numpy(np.load(gold[0])['x'])
    out = {}
    for backbone, ctor in (('resnet18', lambda: resnet18()), ('densenet18', lambda: densenet18(drop_rate=0))):
        m = CNNLinearNetwork(ctor(), 20, 0)
        p = {k: torch.from_numpy(v) for k, v in seeded_params(backbone, 5).items()}
        m.load_state_dict(p, strict=False)
        with torch.no_grad():
            out[backbone] = m.train()(x, None).numpy()
            assert torch.equal(torch.from_numpy(out[backbone]), torch_ref.cnn_linear(p, x, backbone))
    np.savez(os.path.join(OUT, 'ref_import_logits.npz'), x_source=os.path.basename(gold[0]), **out)


if __name__ == '__main__':
    main(sys.argv[1])
