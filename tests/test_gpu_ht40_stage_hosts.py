"""tests/cxx/rx_ht40_chain.cpp -- a C++ host that runs one described 40 MHz HT frame through the adapters of include/sora_brick.hpp for the 40 MHz stages
(THipHt40DataSymbol, THipHt40MimoEst, THipHt40MimoComp, THipHt40PilotTrack, THipHt40Demap, THipHt40Deinterleave, with THipFFT128 between them) and the trellis, the
descrambler and the sink -- built and run on the GPU: the theta it ends with, both rows' error code and FCS and the checksum of its soft bytes equal the handle's for
the same frame.  The adapters also instantiate without a GPU (the syntax check below needs none, but lives here with its host)."""
import os

import numpy as np
import pytest

import ht40_stage_model as sm
from ht40_soft_check import soft_capacity
from test_ht40_data_model import send

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "rx_ht40_chain.cpp")


def test_the_adapters_instantiate():
    import subprocess
    text = open(SRC).read()
    for name in ("THipHt40DataSymbol", "THipHt40MimoEst", "THipHt40MimoComp", "THipHt40PilotTrack", "THipHt40Demap", "THipHt40Deinterleave"):
        assert name + "<" in text, name
    probe = '#include "sora_brick.hpp"\nusing namespace sora_brick;\nCF_Error e;\n' \
            'THipHt40StreamJoin<4, 3, CF_Error, TDrop<CF_Error>> j(e, nullptr, nullptr);\nTHipHt40NoiseVar<CF_Error, TDrop<CF_Error>> v(e, nullptr, nullptr);\n' \
            'static_assert(decltype(j)::oport_traits::burst == 216 * 4 * 3 && decltype(v)::iport_traits::burst == 256, "");\nint main() { return 0; }\n'
    for args in ([SRC], ["-x", "c++", "-"]):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + args, input=probe if args[-1] == "-" else None,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("nb,cr,lens,nv,cfo_step", [(6, 2, (90, 33), 0.5625, 21.0), (1, 0, (30, 41), 0.0, 0.0)])
def test_rx_ht40_chain_host(tmp_path, nb, cr, lens, nv, cfo_step):
    import torch
    import sora_amd
    from test_gpu_hosts import build, run
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    rng = np.random.default_rng(50 + nb)
    iq, ps, _, nsym = send(rng, nb, cr, lens, 6.0, cfo_step=cfo_step, lead=0)
    desc = (0, nb, cr, lens[0], lens[1], int(round(-cfo_step)), nv)
    rx = sora_amd.RxHt40(1, soft_capacity(sora_amd, [desc]))
    t = rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), [desc])
    rows = rx.results(ticket=t); soft = np.concatenate([rx.soft(0, s, ticket=t) for s in range(2)])
    rx.close()
    path = tmp_path / "frame.i16"
    np.ascontiguousarray(iq).tofile(str(path))                                  # chain 0's samples, then chain 1's
    out = run([build("g++", "-std=c++17", SRC, "rx_ht40_chain"), str(path)] + [str(v) for v in desc[1:]])
    f = dict(l.split("=", 1) for l in out.split() if "=" in l)
    sum_ = 0
    for b in soft.tolist():
        sum_ = (sum_ * 31 + b) & 0xFFFFFFFF
    assert int(f["nsym"]) == nsym == rows[0]["nsym"]
    for s in range(2):
        assert (int(f["error%d" % s], 16), int(f["fcs%d" % s], 16)) == (rows[s]["error_code"], rows[s]["crc32"]), (f, rows[s])
        assert rows[s]["error_code"] == 1 and rows[s]["mpdu"] == ps[s]
    assert int(f["soft_checksum"], 16) == sum_, f
    assert int(f["theta"]) == int(sm.by_stages(iq, [desc])["theta"][0][-1]), f   # (the handle does not export theta: the model's, which the soft bytes above already depend on)
