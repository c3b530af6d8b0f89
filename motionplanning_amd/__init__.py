from . import collision  # noqa: F401
from . import gridfield  # noqa: F401
from . import gridmap  # noqa: F401
from . import reeds_shepp  # noqa: F401
from . import roadmap  # noqa: F401
