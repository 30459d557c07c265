"""The automaton shapes of the multi-frame streaming step (tests/test_gpu_step_frames.py; tests/test_stream_frames_cpu.py proves on the CPU
that a burst of the automaton equals the slice of its frame-by-frame run).  The references are the existing ones: step_wide_cases ("wide":
17..256 streams of 6 or 8 frames) and, for the bursts longer than that, ant_step_cases ("step": the same automaton, 16 streams of 40 or 24
frames).  A shape takes the first n streams of its reference - streams are independent - and drives sum(bursts) frames."""

# id: (source, reference case, streams, bursts)
SHAPES = {
    "n1-K1": ("wide", "L1-C12", 1, (1,) * 8),                   # lanes past n masked in every tile
    "n1-K2": ("wide", "L1-C12", 1, (2,) * 4),
    "n16-K8": ("wide", "L1-C12", 16, (8,)),                     # one full tile
    "n17-K8": ("wide", "L1-C12", 17, (8,)),                     # tile tail of one
    "n37-K3-3-2": ("wide", "L4-C12", 37, (3, 3, 2)),            # K changes with the state carried
    "n8-K32": ("step", "L4-C12", 8, (32,)),                     # 256 rows exactly, three ways
    "n16-K16": ("step", "L4-C12", 16, (16, 16)),
    "n256-K1": ("wide", "L3-C22", 256, (1,) * 6),
    "n40-K6-C86": ("wide", "L8-C86", 40, (6,)),                 # six class tiles
    "n33-K6-L32": ("wide", "L32-C12", 33, (6,)),                # the largest anticipation head
}
