"""Setting A/B switches by name, for the tools that take the names from their command line.  A switch is a class attribute
of the model (the declaration blocks at the top of ModelBase, nic.NIC and lc_nic.NIC); a dropout rate (r_in, r_lstm, ...) is
set by its constructor.  Anything else is refused: a misspelt or retired name would measure the default arm twice."""
import inspect


def declared(model):
    """the switch names the model's class declares"""
    cls = type(model)
    plain = lambda k: not (callable(getattr(cls, k)) or isinstance(inspect.getattr_static(cls, k), property))
    return sorted(k for k in dir(cls) if k.islower() and not k.startswith("_") and plain(k))


def set_switches(model, attrs):
    """setattr(model, name, value) for every item of ``attrs``; SystemExit with the declared names on an unknown one"""
    for k, v in attrs.items():
        if not (hasattr(type(model), k) or (k.startswith("r_") and k in vars(model))):
            raise SystemExit(f"{type(model).__module__}.{type(model).__name__} declares no switch or rate {k!r}; "
                             f"its switches: {', '.join(declared(model))}")
        setattr(model, k, v)
    return model
