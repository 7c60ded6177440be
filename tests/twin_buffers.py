"""Buffers of the twin cases in the GPU tests: the same call made once on host buffers and once on device pointers, so that the
two can be required to leave the same bytes.  Inputs are numpy arrays; outputs are rooms of bytes, poisoned and a little larger than
asked, so that a write behind the end shows as a difference too."""
import numpy as np

POISON = 0x5A
MARGIN = 16


class Buffers:
    def __init__(self, on_device):
        self.on_device = on_device
        self.kept = []
        self.rooms = {}

    def _place(self, array):
        flat = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        if not self.on_device:
            return flat, flat.ctypes.data
        import torch
        t = torch.from_numpy(flat).cuda()
        return t, t.data_ptr()

    def put(self, array):
        """an input's pointer (None for no array or an empty one)"""
        if array is None or array.size == 0:
            return None
        held, ptr = self._place(array.copy())
        self.kept.append(held)
        return ptr

    def room(self, name, nbytes):
        """an output's pointer: nbytes and a margin behind them, every byte POISON"""
        held, ptr = self._place(np.full(int(nbytes) + MARGIN, POISON, np.uint8))
        self.rooms[name] = held
        return ptr

    def fetch(self):
        """every output as the bytes it holds now, the margin included"""
        if not self.on_device:
            return {name: held.tobytes() for name, held in self.rooms.items()}
        import torch
        torch.cuda.synchronize()
        return {name: held.cpu().numpy().tobytes() for name, held in self.rooms.items()}


def twins(call):
    """call(buffers, device_pointers) -> (what the call returned, apart from the buffers); runs it on host buffers, then on device
    pointers, requires equal returns and equal bytes in every room, and returns (returned, rooms)."""
    got = []
    for on_device in (False, True):
        b = Buffers(on_device)
        returned = call(b, on_device)
        got.append((returned, b.fetch()))
    (host_ret, host_rooms), (dev_ret, dev_rooms) = got
    assert host_ret == dev_ret, (host_ret, dev_ret)
    assert host_rooms.keys() == dev_rooms.keys()
    for name in host_rooms:
        assert host_rooms[name] == dev_rooms[name], name
    return host_ret, host_rooms
