"""Square binary markers found on the GPU: the detector between `render` and `multicoarse` (the reference asks cv2.aruco,
python/cwipc/registration/multicoarse.py:492-527).  The markers are those of the reference's printable targets: a 5 x 5 payload inside
a one-cell black border.  cwipc_hip_detect_markers (include/cwipc_util_amd/hip_ext.h has the contract) does the work; this module
holds the dictionary type and the adapters to the `MarkerDetector` shape MultiCameraCoarseAruco takes.

The package ships no bit patterns: the user supplies the dictionary, as a JSON file (a list of 5 x 5 lists of 0/1 in id order, 1 = a
white cell) or as an array."""
import json
from typing import Any, List, Sequence, Tuple

import numpy as np

from ..util import cwipc_hip_marker_params, cwipc_hip_detect_markers

__all__ = ['MarkerDictionary', 'detect_markers', 'gpu_marker_detector']


class MarkerDictionary:
    """The payloads of the markers to look for: `words[i]` is marker i's, bit 24 - (5*row + col) the cell at (row, col), set = white."""

    def __init__(self, words: Sequence[int]) -> None:
        self.words = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1))
        if len(self.words) < 1:
            raise ValueError("MarkerDictionary: no markers")
        if (self.words >> np.uint32(25)).any():
            raise ValueError("MarkerDictionary: a payload has 25 bits")

    @classmethod
    def from_bits(cls, bits: Any) -> 'MarkerDictionary':
        """bits: n x 5 x 5 of 0/1, 1 = a white cell."""
        b = np.asarray(bits)
        if b.ndim != 3 or b.shape[1:] != (5, 5) or not np.isin(b, (0, 1)).all():
            raise ValueError("MarkerDictionary: bits must be n x 5 x 5 of 0 and 1")
        weights = np.uint32(1) << np.arange(24, -1, -1, dtype=np.uint32)
        return cls((b.reshape(len(b), 25).astype(np.uint32) * weights).sum(axis=1, dtype=np.uint32))

    @classmethod
    def from_file(cls, path: str) -> 'MarkerDictionary':
        """A JSON file: a list of 5 x 5 lists of 0/1, in id order."""
        with open(path) as f:
            return cls.from_bits(json.load(f))

    def __len__(self) -> int:
        return len(self.words)


def detect_markers(rgb: np.ndarray, dictionary: MarkerDictionary, **params: int) -> Tuple[List[List[List[float]]], List[int]]:
    """(per marker its four (u, v) corners: top-left, top-right, bottom-right, bottom-left of the marker; the markers' ids), sorted by
    id: the `MarkerDetector` shape.  params: the fields of cwipc_hip_marker_params."""
    ids, corners, _found = cwipc_hip_detect_markers(rgb, dictionary.words, cwipc_hip_marker_params(**params))
    return corners.astype(np.float64).tolist(), [int(i) for i in ids]


def gpu_marker_detector(dictionary: MarkerDictionary, **params: int) -> Any:
    """A `MarkerDetector` (multicoarse.py) for MultiCameraCoarseAruco.set_marker_detector."""
    cwipc_hip_marker_params(**params)   # (a wrong name fails here, not at the first image)

    def detect(rgb: np.ndarray) -> Tuple[List[List[List[float]]], List[int]]:
        return detect_markers(rgb, dictionary, **params)

    return detect
