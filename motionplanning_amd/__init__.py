from . import collision  # noqa: F401
