"""What the onnxruntime.InferenceSession look-alikes of FSMN, FireRed, MarbleNet and DFSMN share: the node descriptions, the three
getters a reference script calls before `run`, and the element types at the boundary.  (The Silero wrappers are another interface.)"""
from __future__ import annotations

import numpy as np


class _Meta:
    def __init__(self, name, shape, type_):
        self.name, self.shape, self.type = name, shape, type_


def io_types(io_dtype):
    """io_dtype "float32" | "float16" -> (numpy dtype of the float feeds and fetches, their onnxruntime type string)"""
    if io_dtype not in ("float32", "float16"):
        raise ValueError("io_dtype must be 'float32' or 'float16'")
    return (np.float16, "tensor(float16)") if io_dtype == "float16" else (np.float32, "tensor(float)")


def require_int16(audio):
    """onnxruntime's refusal of an audio feed of another element type, in its words."""
    if audio.dtype != np.int16:
        raise ValueError("Unexpected input data type. Actual: (%s) , expected: (tensor(int16))" % audio.dtype)


class Session:
    """Base of the look-alikes: a subclass sets `_inputs_meta` / `_outputs_meta` (lists of _Meta) and defines `run(output_names, feeds)`."""

    _inputs_meta = _outputs_meta = ()

    def get_inputs(self):
        return list(self._inputs_meta)

    def get_outputs(self):
        return list(self._outputs_meta)

    def get_providers(self):
        return ["VadxMI355XExecutionProvider"]
