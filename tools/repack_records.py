#!/usr/bin/env python
"""Rewrite a TFRecord file of the reference's examples into a packed one (strajnet_amd.data.pack_example: bool features one bit per
element, float32 planes as mask + offsets + non-zero words, the ground truth already centre-cropped; lossless).  Host only, NumPy.

    python tools/repack_records.py IN.tfrecords OUT.tfrecords [--grid 512 --out 256] [--test] [--verify]

--test: inference records (no ground truth; inference.py:84-96).  --verify: unpack every packed example on the CPU again and compare it,
bit for bit, with the decoded original.  Prints one JSON line: examples and bytes in and out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from strajnet_amd import data as D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--out', type=int, default=256)
    ap.add_argument('--test', action='store_true')
    ap.add_argument('--verify', action='store_true')
    ap.add_argument('--check-crc', action='store_true', help='verify the payload CRC of every input record (slow without the built library)')
    a = ap.parse_args()
    if os.path.abspath(a.src) == os.path.abspath(a.dst):
        ap.error('source and destination are the same file')
    stats = {'examples': 0, 'payload_bytes_in': 0, 'payload_bytes_out': 0}

    def packed():
        for rec in D.read_tfrecord(a.src, check_data_crc=a.check_crc):
            ex = D.parse_example(rec)
            pk = D.pack_example(ex, a.grid, a.out, a.test)
            if a.verify:
                got = D.unpack_example_reference(pk, a.grid, a.out, a.test)
                want = D.unpack_example_reference({k: bytes(v) for k, v in ex.items()}, a.grid, a.out, a.test)
                for k in want:
                    if not np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)):
                        raise SystemExit(f'repack_records.py: example {stats["examples"]}, feature {k}: the packed form does not unpack to the original')
            out = D.serialize_example(pk)
            stats['examples'] += 1
            stats['payload_bytes_in'] += len(rec)
            stats['payload_bytes_out'] += len(out)
            yield out
    D.write_tfrecord(a.dst, packed())
    stats['ratio'] = round(stats['payload_bytes_in'] / max(1, stats['payload_bytes_out']), 2)
    print(json.dumps(stats))


if __name__ == '__main__':
    main()
