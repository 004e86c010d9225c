"""CPU-only checks: the C-ABI library builds/loads and exports every symbol include/hypad.h declares; the
parameter catalogue matches the reference's state_dict; host-side module plumbing (no compute calls)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from helpers import load, sub_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hypad_amd import build
    return ctypes.CDLL(build.build())


def test_library_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 45
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/hypad.h but not exported"
    from hypad_amd import _C
    assert set(_C.EXPORTS) == declared
    # ... and nothing else: the product library's dynamic symbol table holds exactly the declared entry points
    # (development aids live in libhypad_hip_dev.so, hypad_amd/build.py)
    import subprocess
    from hypad_amd import build
    nm = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    # EVERY defined dynamic symbol of any kind (functions, weak template instantiations, data, kernel handles): -fvisibility=hidden
    # + csrc/exports.map leave nothing that does not start with hypad_
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def test_abi_version_limits_and_errors(lib):
    assert lib.hypad_abi_version() == 7
    a, b = ctypes.c_int(), ctypes.c_int()
    lib.hypad_limits(ctypes.byref(a), ctypes.byref(b))
    assert a.value >= 150 and b.value >= 20
    lib.hypad_error_string.restype = ctypes.c_char_p
    assert lib.hypad_error_string(0) == b"ok" and b"workspace" in lib.hypad_error_string(-2)


@pytest.mark.parametrize("S", [100, 150, 123, 51])
def test_parameter_catalogue_matches_reference_state_dict(S):
    from hypad_amd import _C
    from oracle import tadgan as ot
    mods = {_C.NET_ENCODER: ot.Encoder(S, 20), _C.NET_DECODER: ot.Decoder(S, 20, True), _C.NET_CRITIC_X: ot.CriticX(S, 20),
            _C.NET_CRITIC_Z: ot.CriticZ(20)}
    for net, m in mods.items():
        cat, total = _C.param_catalogue(net, S, 20, True)
        sd = m.state_dict()
        assert [c[0] for c in cat] == list(sd.keys())
        end = 0
        for name, off, shape in cat:
            assert tuple(sd[name].shape) == tuple(shape), name
            assert off % 4 == 0 and off >= end          # 16-byte aligned, non-overlapping
            end = off + int(np.prod(shape))
        assert total >= end and total % 4 == 0
    cat_e, _ = _C.param_catalogue(_C.NET_DECODER, S, 20, False)
    assert not any("hyperbolic" in c[0] for c in cat_e)


def test_modules_mirror_reference_surface():
    from hypad_amd.models import tadgan
    fx = load("fwd_S100_B64.npz")
    enc, dec = tadgan.Encoder(100, 20), tadgan.Decoder(100, 20, True)
    cx, cz = tadgan.CriticX(100, 20), tadgan.CriticZ(20)
    for m, p in ((enc, "enc"), (dec, "dec"), (cx, "cx"), (cz, "cz")):
        sd = sub_state(fx, p)
        m.load_state_dict(sd)
        assert m._glued()
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k
        # the flat arena really backs the parameters
        name, off, shape = m._catalogue[0]
        assert torch.equal(m._arena[off:off + int(np.prod(shape))].view(shape), sd[name])
        buf = io.BytesIO()
        torch.save(m, buf)                      # the reference checkpoints whole modules (train.py:381-385)
        buf.seek(0)
        m2 = torch.load(buf, weights_only=False)
        assert m2._glued() and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert dec.hyperbolic and hasattr(dec, "hyperbolic_linear") and getattr(dec.hyperbolic_linear.bias, "manifold", None) is not None
    assert not hasattr(tadgan.Decoder(100, 20, False), "hyperbolic_linear")
    # same seed -> same initial weights as the reference construction order (models/tadgan.py, hyrnn_nets.py:155-184)
    from oracle import tadgan as ot
    torch.manual_seed(3)
    a = tadgan.Decoder(100, 20, True)
    torch.manual_seed(3)
    b = ot.Decoder(100, 20, True)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def test_product_path_has_no_cpu_fallback():
    from hypad_amd import _C
    from hypad_amd.models import tadgan
    enc = tadgan.Encoder(100, 20)
    with pytest.raises(_C.HypadError):
        enc(torch.zeros(4, 100))
    import subprocess
    import sys
    # nothing under hypad_amd/ may import the oracle
    out = subprocess.run(["grep", "-rl", "--include=*.py", "-E", r"^\s*(from|import) oracle", os.path.join(ROOT, "hypad_amd")],
                         capture_output=True, text=True).stdout.strip()
    assert out == "", out


def test_train_module_keeps_the_reference_call_surface():
    """train.py:18,107,189,252,409 signatures (positional order the reference's callers use), plus the north_star's
    `encoder_iteration` name for the generator step."""
    import inspect
    from hypad_amd import train as ht
    lead = lambda f, n: list(inspect.signature(f).parameters)[:n]
    assert lead(ht.critic_x_iteration, 5) == ["sample", "decoder", "critic_x", "optim_cx", "params"]
    assert lead(ht.critic_z_iteration, 5) == ["sample", "encoder", "critic_z", "optim_cz", "params"]
    assert lead(ht.decoder_iteration, 8) == ["sample", "encoder", "decoder", "critic_x", "critic_z", "optim_dec", "params", "err_loss"]
    assert lead(ht.encoder_iteration, 5) == ["sample", "encoder", "decoder", "critic_x", "critic_z"]
    assert lead(ht.train_tadgan, 8) == ["train_loader", "encoder", "decoder", "critic_x", "critic_z", "n_epochs", "params", "path"]
    assert lead(ht.train, 3) == ["train_loader", "params", "config_path"]


def test_wide_buffer_stores_keep_their_offset_out_of_scalar_registers():
    """gfx950 needs a wait state between `buffer_store_dwordx4 ..., s_off offen` and a VALU write of its data registers, and
    hipcc (ROCm 7.2) inserts none for that form (profiles/r03_store16_hazard.txt; csrc/tile_gemm.h GBuf::st4): every 12- / 16-byte
    raw buffer store of the kernel sources must pass the literal 0 as its scalar offset (the compiler pads the immediate form)."""
    import glob
    pat = re.compile(r"__builtin_amdgcn_raw_buffer_store_b(?:96|128)\s*\(")
    found = 0
    for path in glob.glob(os.path.join(ROOT, "hypad_amd", "csrc", "*")):
        if path.endswith("diag.hip"):
            continue                                   # (the reproducer writes the hazardous form on purpose, in inline assembly)
        src = open(path).read()
        for m in pat.finditer(src):
            depth, i, args, cur = 1, m.end(), [], ""
            while depth:
                c = src[i]
                if c == "(":
                    depth += 1
                elif c == ")":
                    depth -= 1
                    if depth == 0:
                        break
                if c == "," and depth == 1:
                    args.append(cur.strip()); cur = ""
                else:
                    cur += c
                i += 1
            args.append(cur.strip())
            assert len(args) == 5 and args[3] == "0", (os.path.basename(path), args)
            found += 1
    assert found >= 3


def test_results_table_follows_the_reference(tmp_path, monkeypatch):
    """utils/anomaly_detection_utils.py:112-126 (host-only part of the mirror): one [signal, tn, fp, fn, tp] row per signal in
    ./results/<params.filename>, created with its header, never duplicated for a signal already present."""
    from types import SimpleNamespace
    import pandas as pd
    adu = pytest.importorskip("hypad_amd.utils.anomaly_detection_utils")
    monkeypatch.chdir(tmp_path)
    P = SimpleNamespace(filename="out.csv", signal="a")
    f = adu.save_result(P, "a", [5, 1, 2, 7])
    adu.save_result(P, "a", [9, 9, 9, 9])                                       # same signal: kept as it was
    P.signal = "b"
    adu.save_result(P, "b", [0, 0, 0, 0])
    t = pd.read_csv(f)
    assert list(t.columns) == ["signal", "tn", "fp", "fn", "tp"] and t.values.tolist() == [["a", 5, 1, 2, 7], ["b", 0, 0, 0, 0]]


def test_product_library_reads_no_environment_variable():
    """SURVEY.md 8b "no hidden state": which kernels a C-ABI call launches depends on its arguments alone.  The A/B switches of the
    training epoch are hypad_epoch_io.flags bits; tuning knobs exist in the development library only (HYPAD_TUNE_INT, -DHYPAD_DIAG=1)."""
    import glob
    for path in glob.glob(os.path.join(ROOT, "hypad_amd", "csrc", "*")):
        if path.endswith("diag.hip"):
            continue
        src = open(path).read()
        uses = [m.start() for m in re.finditer(r"getenv", src)]
        if path.endswith("device_utils.h"):
            block = src[src.index("#if HYPAD_DIAG\n#include <cstdlib>"): src.index("#define HYPAD_TUNE_INT(name, dflt) (dflt)")]
            assert all(block in src and src.index(block) <= u < src.index(block) + len(block) for u in uses)
        else:
            assert not uses, os.path.basename(path)
    import subprocess
    from hypad_amd import build
    und = subprocess.run(["nm", "-D", "--undefined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und


def test_product_sources_carry_no_overridable_default_and_no_round_switch():
    """tuning knobs exist in the development library only.  No kernel source holds a default that a -D on the compiler's
    command line can change (`#ifndef HYPAD_X` / `#define HYPAD_X value`: a measured decision is a constexpr, an experiment brings its own
    switch on its own branch through scripts/ab_variants.sh), nor a round's A/B switch (HYPAD_R<n>_...).  A header's include guard defines
    its name to nothing and is not meant."""
    import glob
    default = re.compile(r"^[ \t]*#[ \t]*(?:ifndef[ \t]+|if[ \t]+![ \t]*defined[ \t]*\(?[ \t]*)(HYPAD_\w+)[^\n]*\n(?:[ \t]*\n)*[ \t]*#[ \t]*define[ \t]+\1[ \t]+(?!/[/*])\S", re.M)
    paths = [p for p in glob.glob(os.path.join(ROOT, "hypad_amd", "csrc", "*")) if not p.endswith("diag.hip")]
    assert len(paths) >= 15
    for path in paths:
        src = open(path).read()
        assert not [m.group(1) for m in default.finditer(src)], os.path.basename(path)
        assert not re.findall(r"\bHYPAD_R\d+_\w*", src), os.path.basename(path)
    guard = "#ifndef HYPAD_TILE_GEMM_H\n#define HYPAD_TILE_GEMM_H   // include guard\n#endif\n"
    assert not default.search(guard) and default.search("#ifndef HYPAD_KNOB\n#define HYPAD_KNOB 4\n#endif\n") and default.search("  #if !defined(HYPAD_KNOB)\n\n  # define HYPAD_KNOB (2)\n")


def test_shared_kernel_bodies_are_included_by_two_kernels():
    """a single-signal scoring kernel and its segmented twin share their body as text, csrc/<name>_body.inc, included
    inside both.  Every fragment is included inside at least two different kernels (one included once, or orphaned by a later edit,
    is just an indirection), and every `#include "... .inc"` names a fragment that exists."""
    import glob
    csrc = os.path.join(ROOT, "hypad_amd", "csrc")
    fragments = {os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.inc"))}
    assert fragments
    users = {f: set() for f in fragments}
    for path in glob.glob(os.path.join(csrc, "*")):
        src = open(path).read()
        for m in re.finditer(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+\.inc)"', src, re.M):
            assert m.group(1) in fragments, (os.path.basename(path), m.group(1))
            # the kernel the directive sits in: the last `__global__ ... void name(` in front of it
            kernels = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src[:m.start()], re.S)
            assert kernels, (os.path.basename(path), m.group(1))
            users[m.group(1)].add(kernels[-1])
    assert all(len(k) >= 2 for k in users.values()), {f: sorted(k) for f, k in users.items() if len(k) < 2}


def test_every_translation_unit_is_built():
    """The weights-stationary T = 1 LSTM forwards have their own file (csrc/lstm_t1_lds.hip), which hypad_lstm_bidir_fwd of
    ops_dense.hip calls into: it is in the product library's source list, and so is every other csrc/*.hip but the development
    library's diag.hip (a file left out would only show as an undefined symbol when the library is loaded)."""
    import glob
    from hypad_amd import build
    assert "lstm_t1_lds.hip" in build.SOURCES
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "hypad_amd", "csrc", "*.hip"))}
    assert on_disk - {"diag.hip"} == {s for s in build.SOURCES if s.endswith(".hip")}
    assert on_disk == {s for s in build.DEV_SOURCES if s.endswith(".hip")}


def test_no_scratch_in_the_kernels_the_baseline_configs_run():
    """Code-object metadata of the built gfx950 objects (hypad_amd.build.kernel_metadata: the notes hipcc wrote): the kernels the BASELINE
    configs launch -- every compile-time instantiation of configs[0..2]'s shape (window 100, latent 20, batch 64), the generator / dW / scoring
    kernels of configs[3] and [4] -- spill no vector register and use no scratch memory.  Known gap, held to its current size so that it
    can only shrink: critic_persistent_kernel<150, 20, 256> (configs[3]'s resident critic launch: at most 29 spilled registers and 120 bytes
    of scratch).  Run-time-shape fallbacks (<0, 0, 0>) are not held to anything here."""
    from hypad_amd import build
    build.build()
    ks = []
    for f in sorted(os.listdir(build.LIB_DIR)):
        if f.endswith(".o"):
            ks += build.kernel_metadata(os.path.join(build.LIB_DIR, f))
    assert len(ks) > 100
    by_name = {k["name"]: k for k in ks}
    clean = [n for n in by_name if any(t in n for t in ("<100, 20, 64>", "<true, 100, 20, 64", "<false, 100, 20, 64", "<100, 20>", "<150, 20, 256, ", "<true, 150, 20, 256>",
                                                        "<100, 20, 64, ", "<123, 20, 64", "<51, 20, 64", "<true, 123, 20, 64>", "<true, 51, 20, 64>", "<123, 20>", "<51, 20>", "kde_mode_kernel", "score_forward_packed", "critic_rows_kernel", "lstm_fwd_lds2_kernel", "lstm_fwd_lds3_kernel",
                                                        "dtw_error_kernel", "rolling_mean_kernel", "qs_level_kernel", "unary_rows", "rowdist_rows", "mobius_add_rows",
                                                        "pack_generator_kernel", "epoch_shuffle_kernel", "decay_steps_kernel"))]
    clean += [n for n in by_name if "unroll_median_kernel" in n and ", 128>" in n]           # (the tile size every launch uses)
    assert len(clean) >= 25, sorted(clean)
    for must in ("critic_persistent_kernel<100, 20, 64>", "critic_iteration_kernel<100, 20, 64>", "gen_kernel<true, 100, 20, 64>", "gen_kernel<true, 150, 20, 256>",
                 "dw_adam_kernel<100, 20, 64, 48", "critic_phase_precompute_kernel<100, 20>", "kde_mode_kernel<2>", "score_forward_packed_kernel<100, 20, 2>",
                 "critic_rows_kernel<100, 20>",
                 # the reference's shipped multivariate shapes (configs/multivariate.yaml:5-7: WADI 123, SWAT 51; batch 64)
                 "critic_persistent_kernel<123, 20, 64>", "critic_persistent_kernel<51, 20, 64>", "critic_iteration_kernel<123, 20, 64>",
                 "critic_iteration_kernel<51, 20, 64>", "gen_kernel<true, 123, 20, 64>", "gen_kernel<true, 51, 20, 64>", "dw_adam_kernel<123, 20, 64, 48",
                 "dw_adam_kernel<51, 20, 64, 48", "critic_phase_precompute_kernel<123, 20>", "critic_phase_precompute_kernel<51, 20>"):
        assert any(must in n for n in clean), must
    # (dw_adam_kernel<.., 48, false>, the spread placement: no spilled vector register and not one scratch instruction in its code, but the
    # register allocator reserves a 20-byte emergency slot for its 68 spilled scalars -- allowed, as a reservation of at most 32 bytes)
    reserve = lambda n: 32 if any(("dw_adam_kernel<%s, 48" % t) in n for t in ("150, 20, 256", "100, 20, 64", "123, 20, 64", "51, 20, 64")) else 0
    bad = {n: (by_name[n]["vgpr_spill_count"], by_name[n]["private_segment_fixed_size"]) for n in clean
           if by_name[n]["vgpr_spill_count"] or by_name[n]["private_segment_fixed_size"] > reserve(n)}
    assert not bad, bad
    # ... and NOTHING else in the product library spills a vector register or owns scratch, except the two run-time-shape fallbacks of the critic phase
    # (<0, 0, 0>: any window / latent / batch the compile-time list does not name) and the gap below
    others = {n: (k["vgpr_spill_count"], k["private_segment_fixed_size"]) for n, k in by_name.items()
              if (k["vgpr_spill_count"] or k["private_segment_fixed_size"] > reserve(n)) and "<0, 0, 0>" not in n and "critic_persistent_kernel<150, 20, 256>" not in n}
    assert not others, others
    gap = [k for n, k in by_name.items() if "critic_persistent_kernel<150, 20, 256>" in n]
    assert len(gap) == 1 and gap[0]["vgpr_spill_count"] <= 29 and gap[0]["private_segment_fixed_size"] <= 120, gap   # (29: the hoisted reciprocals, 10.14 -> 10.09 ms per epoch with them)


def test_design_document_stays_readable():
    """DESIGN.md is the CURRENT design -- at most 40 KB, lines of at most 160 characters; the round-by-round record lives
    under docs/history/."""
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path, encoding="utf-8").read()
    assert len(text.encode("utf-8")) <= 40 * 1024
    assert max(len(line) for line in text.splitlines()) <= 160
    assert os.path.exists(os.path.join(ROOT, "docs", "history", "DESIGN_rounds1-5.md")) and os.path.exists(os.path.join(ROOT, "docs", "history", "round6.md"))
    for section in ("## 0. Scope", "## 1. The path and its boundary", "## 2. Oracle and parity", "## 3. Data layout in HBM", "## 4. Kernels", "## 5. Measurement",
                    "## 6. Multi-GPU", "## 7. Next components", "## 8. Status"):
        assert section in text, section


def test_dense_entry_points_validate_their_arguments_before_any_hip_call(lib):
    """No GPU needed: each of these is refused by the argument checks, which come before the first HIP call of the entry point (on a
    machine without a device anything later returns a HIP error code instead).  hypad_linear_act_bwd used to find "grad_bias without
    grad_weight" only after it had launched the data kernel."""
    buf = (ctypes.c_float * 4096)()
    p, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
    # (x, w, y, gy, gx, gw, gb, gpre, rows, K, N, act, stream): a bias gradient without a weight gradient
    assert lib.hypad_linear_act_bwd(p, p, p, p, p, None, p, p, n64(4), 3, 2, 0, None) == EINVAL
    assert lib.hypad_linear_act_bwd(p, p, None, p, p, p, p, p, n64(4), 3, 2, 1, None) == EINVAL           # tanh needs y
    assert lib.hypad_linear_act_bwd(p, p, p, p, p, p, p, None, n64(4), 3, 2, 0, None) == EINVAL           # grad_weight needs the scratch
    # out_dim 257 > 64 * MAX_EPL; a workspace one float short of hypad_mobius_linear_workspace_bytes(4, 2)
    assert lib.hypad_mobius_linear_fwd(p, p, p, p, None, n64(4), 3, 257, None) == EUNSUPPORTED
    lib.hypad_mobius_linear_workspace_bytes.restype = ctypes.c_size_t
    need = lib.hypad_mobius_linear_workspace_bytes(n64(4), 2)
    assert need == 4 * 2 * 2 * 4
    assert lib.hypad_mobius_linear_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(need - 4), n64(4), 3, 2, None) == EWORKSPACE
    assert lib.hypad_mobius_linear_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(1 << 20), n64(4), 3, 257, None) == EUNSUPPORTED
    assert lib.hypad_mobius_head_bwd(p, p, p, p, None, n64(4), 257, None) == EUNSUPPORTED


def test_lstm_seq_and_optimizer_entry_points_validate_their_arguments_before_any_hip_call(lib):
    """No GPU needed.  The general-T LSTM layer accepts the empty batch like every other layer entry point: rows == 0 returns HYPAD_OK
    from the two forwards with NULL row buffers and a NULL zero-byte workspace (nothing to write, no HIP call); the backward's zeroing
    of the parameter gradients is a HIP call and is checked on the GPU (tests/test_gpu_lstm_seq.py).  seq_len <= 0, rows < 0, a NULL
    parameter and hidden > 64 are refused before that.  The stand-alone optimizer steps refuse a ball wider than 256, a ball that does
    not fit, step < 1 and NULL buffers, and accept n == 0."""
    buf = (ctypes.c_float * 4096)()
    p, n64, sz, f = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
    OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
    lib.hypad_lstm_seq_workspace_bytes.restype = lib.hypad_lstm_seq_bwd_workspace_bytes.restype = ctypes.c_size_t
    assert lib.hypad_lstm_seq_workspace_bytes(3, n64(0), 20) == 0 and lib.hypad_lstm_seq_bwd_workspace_bytes(3, n64(0), 12, 20) == 0
    w8 = [p] * 8
    fwd = lambda rows, T=3, ws=None, params=w8, H=20: lib.hypad_lstm_bidir_seq_fwd(None, *params, None, None, None, None, None, T, n64(rows), 12, H,
                                                                                 ws, sz(0), None)
    trn = lambda rows, T=3, ws=None, params=w8, H=20: lib.hypad_lstm_bidir_seq_fwd_train(None, *params, None, None, None, None, None, None, T,
                                                                                       n64(rows), 12, H, ws, sz(0), None)
    for call in (fwd, trn):
        assert call(0) == OK
        assert call(0, T=0) == EINVAL and call(0, T=-1) == EINVAL and call(-1) == EINVAL
        assert call(0, params=[p] * 3 + [None] + [p] * 4) == EINVAL
        assert call(0, H=65) == EUNSUPPORTED
        assert call(4) == EINVAL                                           # rows without x / out
    # (x, w_ih_f, w_hh_f, w_ih_r, w_hh_r, h0, c0, out, saved, grad_out, grad_hn, grad_cn, grad_x, six parameter gradients, grad_h0, grad_c0, ...)
    bwd = lambda rows, T=3, H=20, gw=p, ws=None, nws=0, rowbuf=None: lib.hypad_lstm_bidir_seq_bwd(
        rowbuf, p, p, p, p, None, None, rowbuf, rowbuf, rowbuf, None, None, rowbuf, p, gw, p, p, p, p, None, None, T, n64(rows), 12, H, ws, sz(nws), None)
    assert bwd(0, T=0) == EINVAL and bwd(-1) == EINVAL and bwd(0, gw=None) == EINVAL and bwd(0, H=65) == EUNSUPPORTED
    assert bwd(4) == EINVAL                                                # rows without the row buffers
    assert bwd(4, rowbuf=p) == EWORKSPACE and bwd(4, rowbuf=p, ws=p, nws=64) == EWORKSPACE
    # (p, g, m, v, n, step, lr, b1, b2, eps, wd, stream) / (p, g, m, v, n, ball_off, ball_dim, step, lr, b1, b2, eps, wd, stabilize, stream)
    hp = (f(0.05), f(0.9), f(0.999), f(1e-8), f(0.0))
    adam = lambda a=p, n=8, step=1: lib.hypad_adam_step(a, p, p, p, n64(n), step, *hp, None)
    radam = lambda a=p, n=300, off=0, dim=0, step=1: lib.hypad_radam_step(p, a, p, p, n64(n), n64(off), dim, step, *hp, 10, None)
    assert adam(n=0) == OK and adam(step=0) == EINVAL and adam(a=None) == EINVAL and adam(n=-1) == EINVAL
    assert radam(n=0) == OK and radam(step=0) == EINVAL and radam(a=None) == EINVAL
    assert radam(dim=257, n=300) == EINVAL and radam(off=45, dim=256) == EINVAL and radam(off=-1, dim=4) == EINVAL


def test_error_kernels_refuse_score_windows_without_an_instantiation_before_any_launch(lib):
    """No GPU needed (fake pointers): hypad_dtw_error has the window lengths 3, 5, 7, 9, 11 and 21 -- score windows 12 and 22 (lengths
    13 and 23) are HYPAD_EUNSUPPORTED, score window 1 is HYPAD_EINVAL for it and for hypad_area_error; an empty series is HYPAD_OK.  All of
    them return before the first HIP call (on a machine without a device anything later returns a HIP error code instead)."""
    buf = (ctypes.c_double * 64)()
    p, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    OK, EINVAL, EUNSUPPORTED = 0, -1, -3
    for sw in (12, 13, 22, 23, 14, 40):
        assert lib.hypad_dtw_error(p, p, p, n64(40), sw, None) == EUNSUPPORTED, sw
    for sw in (1, 0, -3):
        assert lib.hypad_dtw_error(p, p, p, n64(40), sw, None) == EINVAL, sw
        assert lib.hypad_area_error(p, p, p, n64(40), sw, None) == EINVAL, sw
    assert lib.hypad_dtw_error(p, p, p, n64(-1), 10, None) == EINVAL and lib.hypad_area_error(p, p, None, n64(4), 10, None) == EINVAL
    assert lib.hypad_dtw_error(p, p, p, n64(0), 10, None) == OK and lib.hypad_area_error(p, p, p, n64(0), 10, None) == OK


def test_statistics_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """No GPU needed (fake pointers): the rolling mean, the z-scores, the quantiles and their segmented copies return HYPAD_EINVAL,
    HYPAD_EUNSUPPORTED or HYPAD_EWORKSPACE from their argument checks, which come before the first HIP call (on a machine without a
    device anything later returns a HIP error code instead).  An empty series is HYPAD_OK for hypad_rolling_mean alone."""
    buf = (ctypes.c_double * 4096)()
    p, n64, sz, dbl = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64, ctypes.c_size_t, ctypes.c_double
    OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
    big = 1 << 40
    for name in ("hypad_rolling_workspace_bytes", "hypad_quantile_workspace_bytes", "hypad_critic_score_workspace_bytes", "hypad_quantiles_signals_workspace_bytes",
                 "hypad_zscore_clip_signals_workspace_bytes", "hypad_critic_score_signals_workspace_bytes", "hypad_rec_scores_signals_workspace_bytes",
                 "hypad_critic_chain_signals_workspace_bytes"):
        getattr(lib, name).restype = sz
    qs = lambda *v: (dbl * len(v))(*v)
    offs = lambda *v: (n64 * len(v))(*v)
    # hypad_rolling_mean(in, sub, out, t, window, origin, workspace, workspace_bytes, stream)
    roll = lambda a=p, o=p, t=100, w=40, origin=0, ws=p, nb=big: lib.hypad_rolling_mean(a, None, o, n64(t), w, n64(origin), ws, sz(nb), None)
    assert roll(a=None) == EINVAL and roll(o=None) == EINVAL and roll(t=-1) == EINVAL and roll(w=0) == EINVAL and roll(w=-3) == EINVAL and roll(origin=-1) == EINVAL
    assert roll(t=0) == OK and roll(t=0, w=3, ws=None, nb=0) == OK and roll(t=0, ws=None, nb=0) == OK
    need = lib.hypad_rolling_workspace_bytes(n64(100))
    assert roll(ws=None) == EWORKSPACE and roll(nb=need - 1) == EWORKSPACE and roll(w=33, nb=need - 1) == EWORKSPACE
    assert lib.hypad_rolling_workspace_bytes(n64(0)) == 0 and lib.hypad_rolling_workspace_bytes(n64(-5)) == 0
    # ... whose workspace holds the chunk sums and counts of roll_counts(t, origin) at every origin: restated from the two shifts
    for t in range(1, 601):
        n1 = max(((o + t - 1) >> 4) - (o >> 4) + 1 for o in range(512))
        n2 = max(((o + t - 1) >> 8) - (o >> 8) + 1 for o in range(512))
        cap1, cap2 = t // 16 + 3, t // 256 + 3                # (the slots hypad_rolling_mean lays out: sums, then counts)
        assert n1 <= cap1 and n2 <= cap2 and lib.hypad_rolling_workspace_bytes(n64(t)) >= (cap1 + cap2) * (8 + 4), t
    # hypad_zscore_clip(in, out, t, ws, bytes, stream) / hypad_critic_zscore(in, q25, q75, out, t, ws, bytes, stream)
    stats = 256 * 5 * 8
    zs = lambda a=p, o=p, t=100, ws=p, nb=stats: lib.hypad_zscore_clip(a, o, n64(t), ws, sz(nb), None)
    cz = lambda a=p, o=p, t=100, ws=p, nb=stats: lib.hypad_critic_zscore(a, dbl(-1.0), dbl(1.0), o, n64(t), ws, sz(nb), None)
    for call in (zs, cz):
        assert call(a=None) == EINVAL and call(o=None) == EINVAL and call(t=0) == EINVAL and call(t=-1) == EINVAL
        assert call(ws=None) == EWORKSPACE and call(nb=stats - 1) == EWORKSPACE
    # hypad_quantiles(in, n, q, nq, out, ws, bytes, stream)
    qneed = lib.hypad_quantile_workspace_bytes()
    qu = lambda a=p, n=100, q=qs(0.25, 0.75), nq=2, o=p, ws=p, nb=qneed: lib.hypad_quantiles(a, n64(n), q, nq, o, ws, sz(nb), None)
    assert qu(a=None) == EINVAL and qu(q=None) == EINVAL and qu(o=None) == EINVAL and qu(n=0) == EINVAL and qu(n=-1) == EINVAL and qu(nq=0) == EINVAL
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert qu(q=qs(0.5, bad)) == EINVAL and qu(q=qs(bad), nq=1) == EINVAL, bad
    assert qu(q=qs(0.1, 0.2, 0.3), nq=3) == EUNSUPPORTED and qu(n=(1 << 31) + 1) == EUNSUPPORTED
    assert qu(ws=None) == EWORKSPACE and qu(nb=qneed - 1) == EWORKSPACE
    # hypad_critic_score(in, out, t, ws, bytes, stream)
    cneed = lib.hypad_critic_score_workspace_bytes()
    assert cneed == 64 + stats + qneed
    cs = lambda a=p, o=p, t=100, ws=p, nb=cneed: lib.hypad_critic_score(a, o, n64(t), ws, sz(nb), None)
    assert cs(a=None) == EINVAL and cs(o=None) == EINVAL and cs(t=0) == EINVAL and cs(t=(1 << 31) + 1) == EUNSUPPORTED
    assert cs(ws=None) == EWORKSPACE and cs(nb=cneed - 1) == EWORKSPACE
    # the segmented copies: the offsets first (n_signals < 1, NULL, a first offset that is not 0, an empty segment)
    ro, W = offs(0, 120, 300), 10
    bad_tables = ((0, ro), (2, None), (2, offs(1, 120, 300)), (2, offs(0, 120, 120)))
    # hypad_quantiles_signals(in, n_signals, row_off, window, q, nq, out, ws, bytes, stream)
    sneed = lib.hypad_quantiles_signals_workspace_bytes(2)
    assert lib.hypad_quantiles_signals_workspace_bytes(0) == 0 and sneed > 0
    qss = lambda a=p, k=2, r=ro, w=W, q=qs(0.25, 0.75), nq=2, o=p, ws=p, nb=sneed: lib.hypad_quantiles_signals(a, k, r, w, q, nq, o, ws, sz(nb), None)
    assert all(qss(k=k, r=r) == EINVAL for k, r in bad_tables)
    assert qss(a=None) == EINVAL and qss(q=None) == EINVAL and qss(o=None) == EINVAL and qss(w=0) == EINVAL and qss(nq=0) == EINVAL and qss(q=qs(0.5, 1.5)) == EINVAL
    assert qss(q=qs(0.1, 0.2, 0.3), nq=3) == EUNSUPPORTED and qss(r=offs(0, 120, 121 + (1 << 31))) == EUNSUPPORTED
    assert qss(ws=None) == EWORKSPACE and qss(nb=sneed - 1) == EWORKSPACE
    # hypad_zscore_clip_signals(in, out, n_signals, seg_off, ws, bytes, stream)
    zneed = lib.hypad_zscore_clip_signals_workspace_bytes(2)
    assert zneed == 2 * stats and lib.hypad_zscore_clip_signals_workspace_bytes(0) == 0
    zss = lambda a=p, o=p, k=2, r=ro, ws=p, nb=zneed: lib.hypad_zscore_clip_signals(a, o, k, r, ws, sz(nb), None)
    assert all(zss(k=k, r=r) == EINVAL for k, r in bad_tables) and zss(a=None) == EINVAL and zss(o=None) == EINVAL
    assert zss(ws=None) == EWORKSPACE and zss(nb=zneed - 1) == EWORKSPACE
    # hypad_critic_score_signals(modes, out, n_signals, row_off, window, ws, bytes, stream)
    csneed = lib.hypad_critic_score_signals_workspace_bytes(2, ro, W)
    assert csneed > cneed and lib.hypad_critic_score_signals_workspace_bytes(2, ro, 0) == 0 and lib.hypad_critic_score_signals_workspace_bytes(0, ro, W) == 0
    css = lambda a=p, o=p, k=2, r=ro, w=W, ws=p, nb=csneed: lib.hypad_critic_score_signals(a, o, k, r, w, ws, sz(nb), None)
    assert all(css(k=k, r=r) == EINVAL for k, r in bad_tables) and css(a=None) == EINVAL and css(o=None) == EINVAL and css(w=0) == EINVAL
    assert css(ws=None) == EWORKSPACE and css(nb=csneed - 1) == EWORKSPACE
    # hypad_rec_scores_signals(kinds, true, median, out_point, out_area, out_dtw, n_signals, row_off, window, score_window, ws, bytes, stream)
    rneed = lib.hypad_rec_scores_signals_workspace_bytes(2, ro, W)
    assert rneed > 0 and lib.hypad_rec_scores_signals_workspace_bytes(2, ro, 0) == 0
    rss = lambda kinds=7, y=p, m=p, op=p, oa=p, od=p, k=2, r=ro, w=W, sw=10, ws=p, nb=rneed: lib.hypad_rec_scores_signals(kinds, y, m, op, oa, od, k, r, w, sw, ws, sz(nb), None)
    assert all(rss(k=k, r=r) == EINVAL for k, r in bad_tables)
    assert rss(kinds=0) == EINVAL and rss(kinds=8) == EINVAL and rss(y=None) == EINVAL and rss(m=None) == EINVAL and rss(w=0) == EINVAL
    assert rss(op=None) == EINVAL and rss(oa=None) == EINVAL and rss(od=None) == EINVAL and rss(kinds=1, oa=None, od=None, sw=0, nb=0, ws=None) == EWORKSPACE
    assert rss(sw=1) == EINVAL and rss(kinds=2, sw=1) == EINVAL and rss(sw=12) == EUNSUPPORTED and rss(kinds=3, sw=12, nb=rneed - 1) == EWORKSPACE
    assert rss(ws=None) == EWORKSPACE and rss(nb=rneed - 1) == EWORKSPACE
    # hypad_critic_chain_signals(critic, modes_out, out, n_signals, row_off, window, ws, bytes, stream)
    chneed = lib.hypad_critic_chain_signals_workspace_bytes(2, ro, W)
    assert chneed > 0 and lib.hypad_critic_chain_signals_workspace_bytes(2, ro, 0) == 0
    chs = lambda a=p, mo=None, o=p, k=2, r=ro, w=W, ws=p, nb=chneed: lib.hypad_critic_chain_signals(a, mo, o, k, r, w, ws, sz(nb), None)
    assert all(chs(k=k, r=r) == EINVAL for k, r in bad_tables) and chs(a=None) == EINVAL and chs(o=None) == EINVAL and chs(w=0) == EINVAL
    assert chs(w=257) == EUNSUPPORTED and chs(r=offs(0, 120, 121 + (1 << 31))) == EUNSUPPORTED
    assert chs(ws=None) == EWORKSPACE and chs(nb=chneed - 1) == EWORKSPACE and chs(mo=p, nb=chneed - 1) == EWORKSPACE
