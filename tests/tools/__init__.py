"""Shared test helpers (no fixtures, no pytest settings)."""
