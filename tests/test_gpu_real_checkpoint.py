"""Real-checkpoint check, conditional: when an ESPnet model directory of one of the reference's models is present on
the box (SPEECHCATCHER_MODEL_DIR, or a snapshot under ~/.cache/espnet or ~/.cache/huggingface - what
speechcatcher.load_model downloads: speechcatcher.py:50-57,141-143), the drop-in class must load it and agree with
the oracle port fed the SAME checkpoint on the same audio: token ids exact, scores within the north star's 1e-3 per
hypothesis step.  There is no network in the build / test containers, so this test normally skips; it exists so that
a box that does hold a checkpoint exercises the real-weights path (dims read from config.yaml, stats, token list)."""
import os
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _find_model_dir():
    env = os.environ.get("SPEECHCATCHER_MODEL_DIR")
    if env and Path(env).exists():
        return Path(env)
    from speechcatcher_amd.speech2text_streaming import _CKPT_NAMES
    for root in (Path.home() / ".cache/espnet", Path.home() / ".cache/huggingface/hub"):
        if not root.exists():
            continue
        for cfg in root.rglob("config.yaml"):
            d = cfg.parent
            if any((d / n).exists() for n in _CKPT_NAMES) or any(p.name in _CKPT_NAMES for p in d.glob("exp/*/*.pth")):
                return d
    return None


def test_real_checkpoint_matches_the_oracle_port():
    model_dir = _find_model_dir()
    if model_dir is None:
        pytest.skip("no ESPnet checkpoint on this box (set SPEECHCATCHER_MODEL_DIR)")
    _check_model_dir(model_dir)


@pytest.mark.parametrize("vocab", [1024, 1182])
def test_the_same_check_on_a_synthetic_model_directory(tmp_path, vocab):
    """the code path of the conditional test above, on a model directory written with seeded weights in the ESPnet
    layout (M_DEFAULTS dims: what a config.yaml without sizes builds) - so that the check itself is known to run; also
    at V = 1182, the vocabulary the XL checkpoint is believed to have (read from the checkpoint's shapes)"""
    import dataclasses

    from speechcatcher_amd import synth
    from speechcatcher_amd.config import M_DEFAULTS
    cfg = M_DEFAULTS if vocab == 1024 else dataclasses.replace(M_DEFAULTS, vocab_size=vocab)
    assert _check_model_dir(synth.write_model_dir(tmp_path / "m", cfg, seed=11, stats_kind="meanstd")) == vocab


def _check_model_dir(model_dir):
    model_dir = Path(model_dir)
    from oracle.ref_port import RefPortModel, RefPortStreaming
    from speechcatcher_amd import synth
    from speechcatcher_amd.mel import melscale_fbanks_slaney
    from speechcatcher_amd.speech2text_streaming import (Speech2TextStreaming, config_from_dir, find_checkpoint,
                                                         load_state_dict, load_stats)
    sd = load_state_dict(find_checkpoint(model_dir))
    cfg = config_from_dir(model_dir, sd)
    mean, std = load_stats(model_dir)
    mel = melscale_fbanks_slaney(cfg.n_fft // 2 + 1, 0.0, cfg.sample_rate / 2.0, cfg.n_mels, cfg.sample_rate)
    ora = RefPortStreaming(RefPortModel({k: v.float() for k, v in sd.items() if hasattr(v, "float")}, cfg, mel, mean, std),
                           beam_size=5, use_bbd=True)
    s2t = Speech2TextStreaming(model_dir, beam_size=5, device="cuda", use_bbd=True, result_format="espnet")
    wav = os.environ.get("SPEECHCATCHER_TEST_WAV")
    if wav and Path(wav).exists():
        import wave
        with wave.open(wav, "rb") as w:
            assert w.getframerate() == 16000 and w.getnchannels() == 1 and w.getsampwidth() == 2
            audio = np.frombuffer(w.readframes(min(w.getnframes(), 16000 * 20)), dtype="<i2").astype(np.float32) / 32768.0
    else:
        audio = synth.synth_audio(77, 16000 * 8)     # noise: still a full pass through the trained weights
    chunk, res = 8192, None
    for pos in range(0, len(audio), chunk):
        fin = pos + chunk >= len(audio)
        res = s2t(audio[pos:pos + chunk], is_final=fin, finalize_all=fin)
        ora(audio[pos:pos + chunk], is_final=fin, finalize_all=fin)
    ref = ora.running_hyps
    hyps = s2t.beam_state.hypotheses
    assert [h["yseq"] for h in hyps] == [list(h.yseq) for h in ref]
    steps = max(1, len(ref[0].yseq))
    assert max(abs(a["score"] - b.score) for a, b in zip(hyps, ref)) <= 1e-3 * steps
    assert res is not None
    return cfg.vocab_size
