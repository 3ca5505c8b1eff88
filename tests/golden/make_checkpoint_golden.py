"""Store the reference's trained MimoSimulation checkpoint as fixture parts (tests/test_checkpoint.py).

    python tests/golden/make_checkpoint_golden.py <reference>/MimoSimulation/models/checkpoint/checkpoint.pth

The checkpoint (``{"state_dict": {...}}``, 4.1 MB of float32) is larger than a committed file may be, so its
tensors go, in order and unchanged, into ``mimo_checkpoint.partN.pth`` files of the same format.  A tensor that
does not fit the room left in a part (the two [1, 5000, 64] positional tables) continues under the same key in
the next part, cut along dim 1; ``golden_util.load_mimo_checkpoint`` concatenates the pieces back.
"""
import os
import sys

import torch

PART_BYTES = 900_000      # tensor payload per part: the zip container adds ~200 bytes per tensor
HERE = os.path.dirname(os.path.abspath(__file__))


def main(path):
    sd = torch.load(path, weights_only=True, map_location="cpu")["state_dict"]
    parts, cur, room = [], {}, PART_BYTES

    def close():
        nonlocal cur, room
        parts.append(cur)
        cur, room = {}, PART_BYTES

    for k, v in sd.items():
        while v is not None:
            n = v.numel() * v.element_size()
            if n <= room:
                cur[k], room, v = v.clone(), room - n, None
            elif n > PART_BYTES and v.dim() > 1:
                rows = room // (n // v.shape[1])
                if rows:
                    cur[k], v = v[:, :rows].clone(), v[:, rows:]
                close()
            else:
                close()
    if cur:
        close()
    for i, p in enumerate(parts):
        out = os.path.join(HERE, f"mimo_checkpoint.part{i}.pth")
        torch.save({"state_dict": p}, out)
        print(out, os.path.getsize(out))


if __name__ == "__main__":
    main(sys.argv[1])
