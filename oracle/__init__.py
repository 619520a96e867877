"""CPU oracle for the Shift-GCN hot path — TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this package, and only as the checker / reported CPU baseline. The product path
(``shift-gcn_amd/shiftgcn``) never imports it and fails loudly without its HIP library.

* :mod:`oracle.shift_oracle` — vectorised numpy restatement of the reference CUDA
  temporal-shift extension (``model/Temporal_shift/cuda/shift_cuda_kernel.cu``).
* :mod:`oracle.shift_loops`  — scalar-loop restatement used to pin the vectorised one.
* :mod:`oracle.ref_build`    — build recipe: the reference's own kernel templates compiled for
  the host into ``oracle/_ref/`` (never committed); :mod:`oracle.shift_ref` loads them, and
  ``tests/test_oracle_shift_ref.py`` holds the two restatements equal to them bit for bit.
* :mod:`oracle.model_oracle` — PyTorch-eager CPU restatement of ``model/shift_gcn.py``
  (``tcn``, ``Shift_tcn``, ``Shift_gcn``, ``TCN_GCN_unit``, ``Model``) on top of the
  numpy shift, plus the reference training-step semantics (``main.py``).
* :mod:`oracle.stream_ref`   — float64 torch restatements of the streaming kernels
  (BatchNorm planes, gcn gather / dx-finish, masks, the shift-fused forms).
* :mod:`oracle.stream_cases` — their test's shape table, inputs and launch-chooser mirrors.
* :mod:`oracle.pw_ref`       — float64 torch restatements of the pointwise contractions
  (``sgcn_pw_fwd`` / ``sgcn_pw_dw`` / ``sgcn_pw_fwd_tshift``) through the header's plane
  addressing formula.
* :mod:`oracle.pw_cases`     — their test's shape tables and mirrors of the host choosers
  (``shift-gcn_amd/csrc/pw_forms.hpp``; ``tests/test_launch_forms.py`` holds them equal).

Pinning: see each module's header and DESIGN.md §Oracle.
"""
