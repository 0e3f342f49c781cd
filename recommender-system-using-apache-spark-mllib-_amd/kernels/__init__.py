"""ctypes bindings of libals_hip.so, one module per kernel family (DESIGN.md "Host layout")."""
