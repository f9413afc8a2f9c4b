"""ht40_gi_model.py -- TEST INFRASTRUCTURE: the data field of a 40 MHz HT two-stream frame with a guard-interval kind (sora_ht40_process_dev with SORA_HT40_SHORT_GI on a
descriptor's code rate), from the detection weights on, composed symbol by symbol from tests/ht40_stage_model.py's bricks:

  * the two HT-LTF symbols are 160 samples with a prefix of 32, whatever the kind; data symbol d starts at frame position 320 + pitch d and its 128 useful samples cp further
    on: pitch / cp = 160 / 32 (long) or 144 / 16 (short);
  * per symbol: so_freq_comp11n with the phase rule oracle/so_11n.c::ht40_symbol states, at pos + cp -- delta[k] = (pos + cp + k) cfo, step 8 cfo, theta, every value cast
    through int16, over 16 bursts: the phase of sample n of the frame is n cfo - theta whatever the kind --, then so_fft128 per chain, mimo_comp with the GIVEN weights,
    pilot_inc (effective from the next symbol), demap, deinterleave (and stream_join in the joint coding), then the oracle's T11aViterbi<.., 192, 36> and its
    descrambler / FCS sink.
At the long guard interval this is oracle/ht40_data_model.model, brick by brick (tests/test_ht40_gi_models_cpu.py holds it to that); at the short one and cfo = 0 it is
that model on the re-spaced frame (tx_ht40_gi_model.respace).  It never reads the library under test."""
import numpy as np

from oracle import py_ht40 as m
import ht40_joint_model as J
import ht40_stage_model as sm


class Stream:
    def __init__(self, error_code, crc32, psdu):
        self.error_code, self.crc32, self.psdu = error_code, crc32, psdu


class Result:
    """soft: [stream 0, stream 1] uint8 [nsym * 108 * n_bpsc] (joint: the merged bytes, uint8 [nsym * 216 * n_bpsc]); theta int16 [nsym + 1]; xs int16 [nsym, 2, 128, 2];
    streams: [Stream, Stream] (joint: [Stream]); None entries with decode=False"""
    def __init__(self, soft, theta, xs, streams, nsym):
        self.soft, self.theta, self.xs, self.streams, self.nsym = soft, theta, xs, streams, nsym


def geometry(gi):
    """-> (pitch, cp) of the data symbols"""
    return (144, 16) if gi else (160, 32)


def symbol(O, a, b, pos, cp, cfo, theta):
    """the 128 useful samples at frame position pos + cp of both chains, compensated and transformed -> (y0, y1) int16 [128, 2]"""
    st = np.zeros(24, np.int16)
    for k in range(8):
        st[k] = sm._w16((pos + cp + k) * int(cfo)); st[8 + k] = sm._w16(8 * int(cfo)); st[16 + k] = theta
    _, c0, c1 = O.freq_comp11n(st, a[pos + cp:pos + cp + 128], b[pos + cp:pos + cp + 128])
    return O.fft(c0, 128), O.fft(c1, 128)


def model(iq, offset, n_bpsc, code_rate, length, cfo, weights, gi=0, joint=False, decode=True):
    """iq int16 [2, n, 2]; offset: first sample (cyclic prefix) of HT-LTF 1; length: the two streams' PSDU bytes (joint: the one PSDU's); cfo: the descriptor's phase
    step; weights int16 [4, 128, 2]; gi: 0 long / 1 short.  -> Result"""
    iq = np.asarray(iq)
    assert iq.dtype == np.int16 and iq.ndim == 3 and iq.shape[0] == 2 and iq.shape[2] == 2
    nsym = J.nsym_for(length, n_bpsc, code_rate) if joint else m.nsym_for(list(length), n_bpsc, code_rate)
    pitch, cp = geometry(gi)
    assert 0 <= offset and offset + 320 + pitch * nsym <= iq.shape[1], "the frame does not lie inside the capture"
    a = np.ascontiguousarray(iq[0, offset:offset + 320 + pitch * nsym]); b = np.ascontiguousarray(iq[1, offset:offset + 320 + pitch * nsym])
    w = np.ascontiguousarray(weights, np.int16).reshape(4, 128, 2)
    O = sm.oracle()
    ncb = 108 * n_bpsc
    soft = [np.zeros((nsym, ncb), np.uint8), np.zeros((nsym, ncb), np.uint8)]
    theta = np.zeros(nsym + 1, np.int16); xs = np.zeros((nsym, 2, 128, 2), np.int16)
    th = 0
    for d in range(nsym):
        theta[d] = th
        y0, y1 = symbol(O, a, b, 320 + pitch * d, cp, cfo, th)
        x = sm.mimo_comp(w, y0, y1)
        xs[d, 0], xs[d, 1] = x
        th = int(sm._w16(th + sm.pilot_inc(x[0], x[1])))
        for s in range(2):
            soft[s][d] = sm.deinterleave(sm.demap(x[s], n_bpsc), n_bpsc, s)
    theta[nsym] = th
    if joint:
        merged = sm.stream_join(soft[0], soft[1], n_bpsc).reshape(-1)
        jobs = [(merged, int(length))]; out_soft = merged
    else:
        out_soft = [soft[0].reshape(-1), soft[1].reshape(-1)]
        jobs = [(out_soft[s], int(length[s])) for s in range(2)]
    streams = [None] * len(jobs)
    if decode:
        for i, (sb, ln) in enumerate(jobs):
            dec = O.viterbi_frame_ex(sb, code_rate, ln, 192, 36)
            e, psdu, crc = O.desc_sink(dec, ln)
            streams[i] = Stream(e & 0xFFFFFFFF, crc, psdu.tobytes())
    return Result(out_soft, theta, xs, streams, nsym)
