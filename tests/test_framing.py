"""CPU side of the submission files (strajnet_amd/submission.py): the framing rules in Python (frame_reference, submission_reference,
parse_submission) against each other, against the protobuf runtime built from SUBMISSION_SCHEMA, and against csrc/frame.h compiled for
the host; SubmissionWriter on host FramedWaypoints; and the boundary checks of the cases tests/test_framing_gpu.py puts through the
kernels (tests/_framing_cases.py)."""
import io
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _framing_cases as FC                                                   # noqa: E402
from test_deflate_dyn import _host_compiler                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARINT_EDGES = (0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 32 - 1)
VARINT_BYTES = ('00', '7f', '8001', 'ff7f', '808001', 'ffff7f', '80808001', 'ffffffff0f')       # by the encoding's definition
HEADER = dict(account_name='a@b.c', unique_method_name='strajnet-hip', authors=['A. One', 'B. Two'], description='d' * 200,
              method_link='https://example.org/m')
DEFAULT_HEADER = dict(account_name='', unique_method_name='', authors=[''], description='', method_link='')


def _planes(name, b, k):
    buf, H, W = FC.batch(name)
    n = H * W
    return (buf[b, k * n:(k + 1) * n].tobytes(), buf[b, (8 + k) * n:(9 + k) * n].tobytes(), buf[b, (16 + 2 * k) * n:(18 + 2 * k) * n].tobytes())


@pytest.mark.parametrize('level', FC.LEVELS)
@pytest.mark.parametrize('name', ('small', 'mid', 'long', 'many43', 'many', 'sparse'))
def test_cases_land_on_both_sides_of_their_boundaries(name, level):
    FC.check_boundaries(name, level)


def test_schema_is_the_single_statement_of_the_numbers():
    from strajnet_amd import submission as S
    assert set(S.SUBMISSION_SCHEMA) == {'Waypoint', 'ScenarioPrediction', 'ChallengeSubmission'}
    assert S.SUBMISSION_SCHEMA['Waypoint'] == dict(zip(S.WAYPOINT_FIELDS, (1, 2, 3)))
    assert S.SUBMISSION_SCHEMA['ScenarioPrediction'] == {'scenario_id': 1, 'waypoints': 2}
    assert [k for k, _ in sorted(S.SUBMISSION_SCHEMA['ChallengeSubmission'].items(), key=lambda kv: kv[1])] == [
        'account_name', 'unique_method_name', 'authors', 'affiliation', 'description', 'method_link', 'scenario_predictions']
    assert S.frame_tags() == 0x12 | 0x0A << 8 | 0x12 << 16 | 0x1A << 24


def test_varint_edges():
    from strajnet_amd.submission import pb_varint, parse_submission, submission_reference
    for v, h in zip(VARINT_EDGES, VARINT_BYTES):
        assert pb_varint(v).hex() == h and FC.varint_len(v) == len(h) // 2, v
    with pytest.raises(ValueError):
        pb_varint(-1)
    # stream and id lengths at the edges a file can hold, through the parser
    for n in VARINT_EDGES[:-1]:
        scene = [(b'\x01' * n, b'', b'\x02' * (n // 2))] + [(b'', b'', b'')] * 7
        sid = 's' * min(n, 200)
        h, ids, scenes = parse_submission(submission_reference(DEFAULT_HEADER, [sid], [scene]))
        assert h == DEFAULT_HEADER and ids == [sid] and scenes == [scene], n


@pytest.mark.parametrize('level', FC.LEVELS)
def test_frame_reference_round_trips_through_the_parser(level):
    from strajnet_amd.submission import frame_reference, submission_reference, parse_submission
    ref = FC.check_boundaries('small', level) + FC.check_boundaries('mid', level)
    ids = [f'id{b:03d}' for b in range(len(ref))]
    data = submission_reference(HEADER, ids, ref)
    header, got_ids, scenes = parse_submission(data)
    assert header == HEADER and got_ids == ids and scenes == ref
    at = data.index(frame_reference(ref[0]))                                  # a scene's block stands in the file as it is
    assert data[at - len(ids[0]):at] == ids[0].encode()
    assert submission_reference(DEFAULT_HEADER, [], []).hex() == '0a0012001a002a003200'
    assert parse_submission(b'') == ({}, [], [])
    for cut in (1, 11, len(data) - 1):
        with pytest.raises(ValueError):
            parse_submission(data[:cut] if cut > 1 else b'\x3a')
    with pytest.raises(ValueError):
        submission_reference({'no_such_field': ''}, [], [])
    with pytest.raises(ValueError):
        submission_reference(DEFAULT_HEADER, ['a'], [])


def _message_classes():
    """ChallengeSubmission / ScenarioPrediction / Waypoint as protobuf classes, built from SUBMISSION_SCHEMA (proto2)."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    from strajnet_amd.submission import SUBMISSION_SCHEMA as SC
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name='stj_test_submission.proto', package='stj_test', syntax='proto2')
    kinds = {'Waypoint': {n: (F.TYPE_BYTES, F.LABEL_OPTIONAL, None) for n in SC['Waypoint']},
             'ScenarioPrediction': {'scenario_id': (F.TYPE_STRING, F.LABEL_OPTIONAL, None),
                                    'waypoints': (F.TYPE_MESSAGE, F.LABEL_REPEATED, '.stj_test.Waypoint')},
             'ChallengeSubmission': {n: (F.TYPE_STRING, F.LABEL_OPTIONAL, None) for n in SC['ChallengeSubmission']}}
    kinds['ChallengeSubmission']['authors'] = (F.TYPE_STRING, F.LABEL_REPEATED, None)
    kinds['ChallengeSubmission']['scenario_predictions'] = (F.TYPE_MESSAGE, F.LABEL_REPEATED, '.stj_test.ScenarioPrediction')
    for msg in ('Waypoint', 'ScenarioPrediction', 'ChallengeSubmission'):
        m = fd.message_type.add(name=msg)
        for fname, num in SC[msg].items():
            ty, label, tname = kinds[msg][fname]
            f = m.field.add(name=fname, number=num, type=ty, label=label)
            if tname:
                f.type_name = tname
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName('stj_test.ChallengeSubmission'))


@pytest.mark.parametrize('level', FC.LEVELS)
def test_submission_reference_under_the_protobuf_runtime(level):
    pytest.importorskip('google.protobuf')
    from strajnet_amd.submission import submission_reference, WAYPOINT_FIELDS
    Submission = _message_classes()
    ref = FC.reference_streams('small', level)
    ids = ['637f20cafde22ff8', 'e', 'x' * 130]
    for header in (DEFAULT_HEADER, HEADER):
        data = submission_reference(header, ids, ref)
        msg = Submission()
        msg.ParseFromString(data)
        assert msg.account_name == header['account_name'] and list(msg.authors) == header['authors'] and not msg.HasField('affiliation')
        assert msg.description == header['description'] and msg.method_link == header['method_link']
        assert [sp.scenario_id for sp in msg.scenario_predictions] == ids
        for b, sp in enumerate(msg.scenario_predictions):
            assert len(sp.waypoints) == 8
            for k, wp in enumerate(sp.waypoints):
                got = tuple(getattr(wp, f) for f in WAYPOINT_FIELDS)
                assert got == ref[b][k], (b, k)
                assert tuple(zlib.decompress(s) for s in got) == _planes('small', b, k), (b, k)
        assert msg.SerializeToString() == data
    # the way the reference fills the message (inference.py:160-226) serialises to the same bytes
    msg = Submission(account_name='', unique_method_name='', description='', method_link='')
    msg.authors.extend([''])
    for b, sid in enumerate(ids):
        sp = msg.scenario_predictions.add()
        sp.scenario_id = sid
        for k in range(8):
            wp = sp.waypoints.add()
            for f, s in zip(WAYPOINT_FIELDS, ref[b][k]):
                setattr(wp, f, s)
    assert msg.SerializeToString() == submission_reference(DEFAULT_HEADER, ids, ref)


def test_host_framed_waypoints_answer_like_the_reference():
    from strajnet_amd.submission import frame_reference
    ref = FC.reference_streams('small', 2)
    fw = FC.host_framed(ref)
    assert fw.batch == 3 and fw.cpu() is fw and fw.nbytes == fw.buf.numel() == sum(len(frame_reference(s)) for s in ref)
    for b in range(3):
        assert fw.scene_message(b) == frame_reference(ref[b]) and fw.streams(b) == ref[b]


def test_submission_writer_short_last_batch_and_names(tmp_path):
    from strajnet_amd.submission import SubmissionWriter, submission_reference, parse_submission
    ref = FC.reference_streams('small', 1)
    fw = FC.host_framed(ref)
    ids = ['aa', 'bb', 'cc', 'dd', 'ee']
    f = io.BytesIO()
    w = SubmissionWriter(f)
    w.add_batch(fw, ids[:3])
    w.add_batch(fw, ids[3:])                                                  # the last batch: two ids, three scenes in the buffer
    w.close()
    assert w.scenes == 5 and not f.closed
    assert f.getvalue() == submission_reference(DEFAULT_HEADER, ids, ref + ref[:2])
    with pytest.raises(ValueError):
        SubmissionWriter(io.BytesIO()).add_batch(fw, ids[:4])
    path = tmp_path / SubmissionWriter.shard_name('/data/test/00042-of-00150_new.tfrecords')
    with SubmissionWriter(path, **{k: v for k, v in HEADER.items()}) as w:
        w.add_batch(fw, [b'raw-bytes-id'])
    header, got, scenes = parse_submission(path.read_bytes())
    assert header == HEADER and got == ['raw-bytes-id'] and scenes == ref[:1]
    assert path.name == 'occupancy_flow_submission.binproto-00042-of-00150'
    assert SubmissionWriter.shard_name('00007_new.tfrecords-00007-of-00150') == 'occupancy_flow_submission.binproto-00007-of-00150'
    with pytest.raises(ValueError):
        SubmissionWriter.shard_name('/data/test/00042-of-00150.tfrecords')


_HOST_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "%s"
int main() {
  char kind;
  while (scanf(" %%c", &kind) == 1) {
    if (kind == 'V') {
      unsigned int v;
      if (scanf("%%u", &v) != 1) return 2;
      const uint32_t n = pb_varint_len(v);
      uint8_t* p = (uint8_t*)malloc(n);                     /* exactly its length: a byte too many is out of bounds */
      if (pb_put_varint(p, v) != n) return 4;
      printf("V %%u ", n);
      for (uint32_t i = 0; i < n; ++i) printf("%%02x", p[i]);
      printf("\n");
      free(p);
    } else if (kind == 'L') {
      unsigned int tags, lens[3 * FRM_WAYPOINTS], starts[3 * FRM_WAYPOINTS], dry[3 * FRM_WAYPOINTS];
      if (scanf("%%u", &tags) != 1) return 2;
      for (int j = 0; j < 3 * FRM_WAYPOINTS; ++j) if (scanf("%%u", &lens[j]) != 1) return 2;
      const uint32_t total = frm_scene(lens, tags, (uint8_t*)0, dry);
      uint8_t* out = (uint8_t*)calloc(total ? total : 1, 1);   /* exactly the block */
      if (frm_scene(lens, tags, out, starts) != total) return 4;
      printf("L %%u", total);
      uint32_t at = 0;
      for (int j = 0; j < 3 * FRM_WAYPOINTS; ++j) {
        if (dry[j] != starts[j]) return 4;
        printf(" %%u:", starts[j]);
        for (; at < starts[j]; ++at) printf("%%02x", out[at]);
        at += lens[j];
      }
      printf(" %%u\n", at);
      free(out);
    } else {
      return 3;
    }
  }
  return 0;
}
'''


def host_cases():
    """(input lines, expected lines) for the host program: the varint edges, and scenes of planted lengths framed by frame_reference."""
    from strajnet_amd.submission import frame_reference, frame_tags, pb_varint
    lines = [f'V {v}' for v in VARINT_EDGES]
    want = [f'V {len(pb_varint(v))} {pb_varint(v).hex()}' for v in VARINT_EDGES]
    rng = np.random.default_rng(5)
    edge = [0, 1, 126, 127, 128, 129, 16382, 16383, 16384, 2 ** 21 - 1, 2 ** 21]
    scenes = [[0] * 24, [127] * 24, [41, 41, 39] + [41, 41, 40] + [5458] * 3 + [5458, 5458, 5459] + [0] * 12,      # bodies 127 | 128, 16383 | 16384
              edge + edge + [7, 300], [int(x) for x in rng.integers(0, 40000, 24)], [int(x) for x in rng.integers(0, 200, 24)]]
    for lens in scenes:
        streams = [tuple(bytes(lens[3 * k + i]) for i in range(3)) for k in range(8)]
        blk = frame_reference(streams)
        toks, at, end = [], 0, 0
        for k in range(8):
            body = sum(1 + FC.varint_len(l) + l for l in lens[3 * k:3 * k + 3])
            at += 1 + FC.varint_len(body)
            for i in range(3):
                at += 1 + FC.varint_len(lens[3 * k + i])
                toks.append(f'{at}:{blk[end:at].hex()}')
                at += lens[3 * k + i]
                end = at
        assert at == len(blk)
        lines.append(f'L {frame_tags()} ' + ' '.join(map(str, lens)))
        want.append(f'L {len(blk)} ' + ' '.join(toks) + f' {at}')
    return lines, want


def test_host_build_of_frame_h_agrees_with_frame_reference(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host compiler')
    src, exe = tmp_path / 'frame_host.cpp', tmp_path / 'frame_host'
    src.write_text(_HOST_PROGRAM % os.path.join(ROOT, 'strajnet_amd', 'csrc', 'frame.h'))
    r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', str(src), '-o', str(exe)], capture_output=True, text=True)        # host only
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = host_cases()
    r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split('\n')[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lines[i][:60], g[:300], w[:300])


def test_the_library_states_the_framed_sizes(lib_built):
    from strajnet_amd.submission import compress_sizes, compress_framed_sizes
    for B, H, W in ((1, 16, 16), (3, 64, 64), (32, 256, 256)):
        work, cap = compress_sizes(B, H, W)
        fwork, fcap, words = compress_framed_sizes(B, H, W)
        assert fwork == work and words == 6 * B * 8 + B + 1
        assert cap + 6 * 32 * B <= fcap < cap + 6 * 32 * B + 16 and fcap % 16 == 0
